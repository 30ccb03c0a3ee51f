"""Exact per-draw tests of the HIP samplers: ``sample`` / ``sample_temp_rows`` (decode.hip
sample_kernel + sample_final_kernel) and ``sample_rows`` (sampling.hip sample_topkp_kernel).

The kernels are deterministic (integer-hash noise, argmax), so every draw is compared with the
fp64 reference of tests/_sampler_ref.py by exact equality of the token id; there is no
tolerance on kernel output.  A draw is left out only when the REFERENCE's margin between the
best and the second-best score is at most 1e-3 (far above the kernels' f32 score error), and
at most 1 % of a case's draws may be left out.  Inputs, constants and their reasons:
tests/_sampler_cases.py; tests/test_sampler_ref.py checks on the CPU that the inputs are
decidable and that a kept set off by one token would show.
"""
import numpy as np
import pytest
import torch

from tests import _sampler_cases as C
from tests import _sampler_ref as R

pytestmark = pytest.mark.gpu


def _params(c, gpu, rows=None):
    sel = slice(None) if rows is None else rows
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[sel])).to(device=gpu, dtype=dt)  # noqa: E731
    return (t(c.temps, torch.float32), t(c.top_ps, torch.float32), t(c.top_ks, torch.int32), t(c.seeds, torch.int64),
            t(c.steps, torch.int32))


def run(c, entry: str, gpu, rows=None) -> np.ndarray:
    """Token ids of the case's draws (all, or the index array `rows`) through one entry point."""
    from mxllm.ops import native

    ops = native()
    x = c.base.to(gpu)
    if entry == "sample":
        assert rows is None
        T, seed0, steps = c.sample_call
        out = torch.stack([ops.sample(x, T, seed0, s) for s in steps]).reshape(-1)
    else:
        b = torch.from_numpy(c.b if rows is None else c.b[rows]).to(gpu)
        xr = x.index_select(0, b).contiguous()
        temps, top_ps, top_ks, seeds, steps = _params(c, gpu, rows)
        if entry == "temp_rows":
            assert (c.top_ps >= 1).all() and (c.top_ks <= 0).all()
            out = ops.sample_temp_rows(xr, temps, seeds, steps)
        else:
            out = ops.sample_rows(xr, temps, top_ps, top_ks, seeds, steps)
    assert out.dtype == torch.int64
    return out.cpu().numpy()


def check(c, entry: str, got: np.ndarray) -> None:
    ids, margin, _ = C.expected(c.name)
    dec = margin > C.MARGIN
    left = int((~dec).sum())
    assert left <= C.MAX_OMITTED * c.n, (c.name, left)
    assert got.shape == ids.shape
    assert ((got >= 0) & (got < c.base.shape[1])).all(), (c.name, entry)
    bad = np.nonzero(dec & (got != ids))[0]
    detail = [(int(r), int(c.b[r]), int(c.steps[r]), int(got[r]), int(ids[r]), float(margin[r])) for r in bad[:8]]
    assert bad.size == 0, (f"{c.name} via {entry}: {bad.size} of {int(dec.sum())} decidable draws differ; "
                           f"(draw, row, step, got, want, margin): {detail}")


def run_and_check(name: str, gpu) -> dict:
    c = C.by_name()[name]
    got = {e: run(c, e, gpu) for e in c.entries}
    for e, g in got.items():
        check(c, e, g)
    return got


@pytest.mark.parametrize("name", C.names("entry points"))
def test_entry_points_draw_the_reference_token(gpu, name):
    """sample (row seeds seed + 7919 * row), sample_temp_rows and sample_rows without top-k /
    top-p: V 7 ... 4099 (odd V: unaligned rows and a tail after the 8-wide loop) at three
    temperatures, 128256 and 200003 (more than 64 chunks of 2048: the chunk is recomputed),
    and one sample() call of 1030 rows (second launch of the 1024-row loop)."""
    c = C.by_name()[name]
    got = run_and_check(name, gpu)
    if c.base.shape[0] == 1030:
        ids, margin, _ = C.expected(name)
        for r in (0, 1023, 1024, 1029):
            assert margin[r] > C.MARGIN and got["sample"][r] == ids[r], r


@pytest.mark.parametrize("name", C.names("top-k sets") + C.names("radix depth"))
def test_top_k_sets(gpu, name):
    """Head / tail rows with k = 5, 11, 16 and k at a tie (both tied tokens kept); a flat f32 row
    and its negation whose keys differ only in the last radix digit, k in {1, 8, 500, 999} and
    k >= V / k <= 0 as 'off'."""
    run_and_check(name, gpu)


@pytest.mark.parametrize("name", C.names("top-p sets") + C.names("top-k + top-p sets"))
def test_top_p_sets(gpu, name):
    """Head / tail rows with top_p in the middle of a cumulative-mass gap, T 0.7 and 1.0, alone
    and inside a top-k set."""
    run_and_check(name, gpu)


@pytest.mark.parametrize("name", C.names("zeros"))
def test_negative_zero_ties_with_positive_zero(gpu, name):
    """A top-k / top-p boundary on +0.0 keeps the -0.0 tokens: they are drawn where the
    reference draws them."""
    c = C.by_name()[name]
    got = run_and_check(name, gpu)["rows"]
    ids, margin, _ = C.expected(name)
    nz = C.neg_zero_tokens(c.base[0])
    want = np.isin(ids, nz) & (margin > C.MARGIN)
    assert want.sum() > 0.1 * c.n
    assert np.isin(got[want], nz).all()


@pytest.mark.parametrize("name", C.names("-inf entries"))
def test_rows_with_minus_infinity(gpu, name):
    c = C.by_name()[name]
    for e, got in run_and_check(name, gpu).items():
        assert np.isfinite(R.as_f64(c.base)[c.b, got]).all(), e  # every draw, decidable or not


@pytest.mark.parametrize("name", C.names("mixed batch"))
def test_mixed_batch_rows_equal_their_single_row_calls(gpu, name):
    """One sample_rows launch of greedy, temperature, top-k, top-p and top-k + top-p rows: every
    row equals the reference and the launch that holds that row alone."""
    c = C.by_name()[name]
    got = run_and_check(name, gpu)["rows"]
    alone = np.concatenate([run(c, "rows", gpu, rows=np.array([r])) for r in range(c.n)])
    assert np.array_equal(got, alone)


@pytest.mark.parametrize("name", C.names("greedy ties"))
def test_greedy_ties_pick_the_smallest_index(gpu, name):
    c = C.by_name()[name]
    want = [min(t) for t in c.note["ties"]]
    for e, got in run_and_check(name, gpu).items():  # sample (decode.hip) and sample_rows (sampling.hip)
        assert got.tolist() == want, e


def test_u1_triples_are_rederived():
    """The (seed, step, token) triples of the u == 1.0 cases come out of a bounded search over the
    hash, not out of a trusted constant."""
    assert C.find_u1(1000, 200000, 3) == C.U1_V1000
    assert int(R.hash3(*C.U1_V128K)[0]) >> 8 == 0xFFFFFF


@pytest.mark.parametrize("name", C.names("u == 1.0"))
def test_token_whose_noise_rounds_to_one_is_not_forced(gpu, name):
    """h >> 8 == 0xFFFFFF used to give u == 1.0f and a score of +inf.  The token with that noise
    holds the lowest finite logit, 20 below the maximum: the draw is the reference's, not it."""
    c = C.by_name()[name]
    ids, margin, _ = C.expected(name)
    sel = np.nonzero(c.b == c.note["row"])[0]
    assert (margin[sel] > C.MARGIN).all() and (ids[sel] != c.note["token"]).all()
    for e, got in run_and_check(name, gpu).items():
        assert (got[sel] != c.note["token"]).all(), (e, got[sel])
        assert np.array_equal(got[sel], ids[sel]), e
