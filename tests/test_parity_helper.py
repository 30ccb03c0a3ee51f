"""The per-element parity helper (tests/_parity.py) on the CPU: it accepts a correctly rounded
result and rejects three localized corruptions, each of which the global-norm check it replaces
(``|a - b| / |b| < 1e-2``, tests/test_kernels_gpu.py) accepts -- the record of why it exists."""
import re

import pytest
import torch

from tests import _parity as P
from tests._parity import assert_parity

BOUND = (P.ULP_BF16, 0.0)  # one bf16 ulp, no absolute term: the strictest bound the helper is used with


def _global_norm_ok(out, ref, tol=1e-2):
    o, r = out.double(), ref.double()
    return ((o - r).norm() / r.norm()).item() < tol


@pytest.fixture(scope="module")
def ref_out():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(8, 125000, generator=g, dtype=torch.float64)  # 1,000,000 elements
    return ref, ref.to(torch.bfloat16)


def test_accepts_reference_rounded_to_bf16(ref_out):
    ref, out = ref_out
    assert_parity(out, ref, BOUND)
    assert_parity(out, ref, BOUND, scale="tensor")
    assert _global_norm_ok(out, ref)


def test_rejects_one_element_of_a_million_moved_by_4_ulps(ref_out):
    ref, out = ref_out
    bad = out.clone()
    bits = bad.view(torch.int16)
    bits[6, 17403] += 4  # the bit pattern + 4: four bf16 ulps up in magnitude
    with pytest.raises(AssertionError) as e:
        assert_parity(bad, ref, BOUND, name="y")
    msg = str(e.value)
    assert "1 of 1000000 elements" in msg and "worst at (6, 17403)" in msg
    assert re.search(r"out -?\d", msg) and re.search(r"ref -?\d", msg)
    assert _global_norm_ok(bad, ref)


def test_rejects_one_row_scaled(ref_out):
    ref, out = ref_out
    bad = out.clone()
    bad[7] = (bad[7].float() * 1.02).to(torch.bfloat16)  # e.g. a wrong row in a partial last block
    with pytest.raises(AssertionError) as e:
        assert_parity(bad, ref, BOUND)
    msg = str(e.value)
    assert "worst at (7, " in msg and "first at (7, " in msg
    nbad = int(re.match(r"output: (\d+) of", msg).group(1))
    assert 100000 <= nbad <= 125000  # nearly every element of that row, none elsewhere
    assert _global_norm_ok(bad, ref)


def test_rejects_eight_columns_zeroed(ref_out):
    ref, out = ref_out
    bad = out.clone()
    bad[:, 124992:] = 0  # the last 16-byte chunk of every row never written
    with pytest.raises(AssertionError) as e:
        assert_parity(bad, ref, BOUND)
    assert "64 of 1000000 elements" in str(e.value)
    assert _global_norm_ok(bad, ref)


def test_rejects_non_finite_and_wrong_shape(ref_out):
    ref, out = ref_out
    bad = out.clone()
    bad[3, 5] = float("nan")
    with pytest.raises(AssertionError, match=r"worst at \(3, 5\)"):
        assert_parity(bad, ref, (1.0, 1.0))
    with pytest.raises(AssertionError):
        assert_parity(out[:, :-1], ref, BOUND)


def test_absolute_term_is_relative_to_the_row_or_tensor_max():
    ref = torch.tensor([[1e-6, 1.0], [1e-6, 1e-3]], dtype=torch.float64)
    out = ref.clone()
    out[:, 0] += 1e-5
    assert_parity(out[:1], ref[:1], (0.0, 2e-5))  # row max 1
    with pytest.raises(AssertionError, match=r"worst at \(1, 0\)"):
        assert_parity(out, ref, (0.0, 2e-5))  # row 1's max is 1e-3
    assert_parity(out, ref, (0.0, 2e-5), scale="tensor")


def test_constants_follow_from_the_measurements():
    """chosen = (max(2 rel, one ulp of the output dtype), 2 abs) for every recorded output."""
    names = [n[:-len("_MEASURED")] for n in dir(P) if n.endswith("_MEASURED")]
    assert len(names) >= 15
    for n in names:
        rel, ab = getattr(P, n + "_MEASURED")
        c_rel, c_abs = getattr(P, n)
        ulp = P.ULP_BF16 if rel > 0 else P.ULP_F32  # bf16 outputs round (rel ~ 2^-8), fp32 outputs do not
        assert c_rel == max(2 * rel, ulp), n
        assert c_abs == pytest.approx(2 * ab, rel=5e-3), n
