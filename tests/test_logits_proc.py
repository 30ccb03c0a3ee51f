"""Sampling penalties, logit_bias and log-probabilities (mxllm/ops/decode.py
``adjust_logits_rows`` / ``token_state_update`` / ``logprob_rows``; GPU:
csrc/kernels/logits_proc.hip).

CPU tests: the contract of the PyTorch implementations (evaluation order, which tokens each
penalty covers, bit-exact pass-through, the tie rule).  ``gpu`` tests: the kernels against
those implementations -- the adjusted logits bit for bit, the top lists exactly, the
log-probabilities within ``LOGPROB`` of the fp64 log-softmax of the same inputs.

``python -m tests.test_logits_proc`` prints the measurement behind ``LOGPROB`` again (no GPU).
"""
import functools

import pytest
import torch

from mxllm.ops import decode as dops

from ._parity import ULP_F32, assert_exact, assert_parity

# |out - ref| <= c_rel |ref| + c_abs scale, scale = the row's largest |logit| (tests/_parity.py).
# Measured on the CPU at exactly the inputs of LOGPROB_CASES: the plain fp32 expression
# x - logsumexp(x) over every element of every row against the fp64 log-softmax of the same
# rounded inputs: abs = max |y32 - ref| / scale; the output is f32, so no output rounding (rel 0).
# The bound allows twice each and c_rel never falls below one ulp of f32.
LOGPROB_MEASURED = (0, 1.95e-07)
LOGPROB = (max(2 * LOGPROB_MEASURED[0], ULP_F32), 2 * LOGPROB_MEASURED[1])

LOGPROB_CASES = [(50, torch.float32), (777, torch.bfloat16), (1000, torch.bfloat16), (128256, torch.bfloat16),
                 (50001, torch.float32)]
N_TOP = [-1, 0, 1, 5, 20]


def _unaligned(x: torch.Tensor) -> torch.Tensor:
    """The same [B, V] values, contiguous, starting one element past an aligned allocation."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    out = buf[1:].view(x.shape)
    out.copy_(x)
    return out


@functools.lru_cache(maxsize=None)
def _logprob_case(V: int, dtype):
    """(logits [5, V], ids [5], fp64 log-softmax [5, V], expected top ids per row): computed once."""
    g = torch.Generator().manual_seed(V)
    x = (torch.randn(5, V, generator=g) * 2).to(dtype)
    ids = torch.randint(0, V, (5,), generator=g)
    ref = torch.log_softmax(x.double(), -1)
    order = sorted_ids(x)
    return x, ids, ref, order


def sorted_ids(x: torch.Tensor) -> list[list[int]]:
    """Token ids of every row by (-logit, id): plain Python, independent of torch.sort."""
    out = []
    for row in x.double().tolist():
        out.append(sorted(range(len(row)), key=lambda j: (-row[j], j))[:21])
    return out


def _measure():
    worst = 0.0
    for V, dtype in LOGPROB_CASES:
        x, _, ref, _ = _logprob_case(V, dtype)
        xf = x.float()
        y32 = xf - torch.logsumexp(xf, -1, keepdim=True)
        scale = xf.abs().amax(-1, keepdim=True).double()
        e = ((y32.double() - ref).abs() / scale).max().item()
        print(f"V={V} {dtype}: abs {e:.3g} of the row's largest |logit|")
        worst = max(worst, e)
    print(f"LOGPROB_MEASURED = (0, {worst:.3g})")
    return worst


# --------------------------------------------------------------------------- adjust: inputs
def _adjust_case(V: int, dtype, mix: int):
    """logits [5, V] with +0.0 / -0.0 / negative values at touched and untouched places, a
    6-slot token state (prompt flags, counts up to 7), a bias table (+-100 on a few ids)
    and per-row parameters.  mix 0: no-op (slot -1), presence only, frequency only,
    repetition 1.3, repetition 0.8; mix 1: bias only, everything together (twice, with both
    repetition values), a live slot with nothing to do, a negative presence penalty."""
    g = torch.Generator().manual_seed(1000 * V + mix)
    x = torch.randn(5, V, generator=g) * 3
    x[:, 0:4] = torch.tensor([0.0, -0.0, -1.5, 2.5])
    x[:, V - 4:] = torch.tensor([-0.0, 0.0, -3.0, 0.75])
    x = x.to(dtype)
    n_slots = 6
    prompt = torch.rand(n_slots, V, generator=g) < 0.3
    count = torch.randint(0, 8, (n_slots, V), generator=g) * (torch.rand(n_slots, V, generator=g) < 0.25)
    count[:, 1] = 3  # the -0.0 logit is an output token; the +0.0 at V - 3 too
    count[:, V - 3] = 7
    prompt[:, 0] = False  # +0.0 at 0 and -0.0 at V - 4 stay untouched
    count[:, 0] = 0
    prompt[:, V - 4] = False
    count[:, V - 4] = 0
    prompt[:, 2] = True  # a negative logit seen only in the prompt
    count[:, 2] = 0
    state = count.to(torch.int32) | torch.where(prompt, dops.PROMPT_FLAG, 0).to(torch.int32)
    bias = torch.zeros(n_slots, V)
    for s in range(n_slots):
        ids = torch.randperm(V - 8, generator=g)[:6] + 4
        bias[s, ids] = torch.tensor([100.0, -100.0, 100.0, -100.0, 1.5, -0.25])
    if mix == 0:
        slots = [-1, 3, 0, 5, 2]
        pres = [0.9, 0.7, 0.0, 0.0, 0.0]
        freq = [0.9, 0.0, 0.35, 0.0, 0.0]
        rep = [1.3, 1.0, 1.0, 1.3, 0.8]
        use_bias = False
    else:
        slots = [4, 1, 3, 0, 2]
        pres = [0.0, 0.6, -0.4, 0.0, -1.1]
        freq = [0.0, 1.7, 0.2, 0.0, 0.0]
        rep = [1.0, 1.3, 0.8, 1.0, 1.0]
        use_bias = True
        bias[0].zero_()  # row 3: a live slot with nothing to do
        state[0].zero_()
        bias[2].zero_()  # row 4: presence only
    return x, state, slots, pres, freq, rep, (bias if use_bias else None)


def _untouched(x, state, slots, pres, freq, rep, bias):
    """Mask of the elements that none of steps 2-4 touches."""
    B, V = x.shape
    m = torch.ones(B, V, dtype=torch.bool)
    for b, s in enumerate(slots):
        if s < 0:
            continue
        st = state[s]
        touched = torch.zeros(V, dtype=torch.bool)
        if rep[b] != 1:
            touched |= st != 0
        touched |= (st & dops.COUNT_MASK) > 0
        if bias is not None:
            touched |= bias[s] != 0
        m[b] = ~touched
    return m


def _adjust_scalar(x, state, slots, pres, freq, rep, bias):
    """The contract one element at a time, each operation rounded to f32 through a tensor."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    out = x.float().clone()
    for b, s in enumerate(slots):
        if s < 0:
            continue
        for j in range(x.shape[1]):
            st = int(state[s, j])
            v = out[b, j].clone()
            c = st & dops.COUNT_MASK
            if st != 0 and rep[b] != 1:
                v = v / f(rep[b]) if v > 0 else v * f(rep[b])
            if c > 0:
                v = v - (f(freq[b]) * f(float(c)) + f(pres[b]))
            if bias is not None and bias[s, j] != 0:
                v = v + bias[s, j]
            out[b, j] = v
    return out


# --------------------------------------------------------------------------- CPU: the contract
def test_adjust_semantics_by_hand():
    x = torch.tensor([[2.0, -2.0, 2.0, -2.0, 0.0, -0.0, 1.0, 1.0]])
    F = dops.PROMPT_FLAG
    state = torch.tensor([[F, F, 3, F | 2, 0, 0, 0, 1]], dtype=torch.int32)
    bias = torch.tensor([[0, 0, 0, 0, 0, 0, -100.0, 5.0]])
    y = dops.adjust_logits_rows(x, state, [0], [0.25], [0.5], [2.0], bias)
    # prompt-only tokens: repetition only; output tokens: repetition, then frequency * c + presence
    want = torch.tensor([[1.0, -4.0, 1.0 - 1.75, -4.0 - 1.25, 0.0, -0.0, -99.0, 0.5 - 0.75 + 5.0]])
    assert_exact(y, want)
    assert_exact(y.view(torch.int32)[:, 4:6], x.view(torch.int32)[:, 4:6])  # both zeros keep their sign
    assert_exact(dops.adjust_logits_rows(x.bfloat16(), state, [-1], [0.25], [0.5], [2.0], bias), x)
    # no state at all: bias only
    assert_exact(dops.adjust_logits_rows(x, None, [0], [0.25], [0.5], [2.0], bias), x + bias)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("mix", [0, 1])
def test_adjust_cpu_matches_scalar_contract(dtype, mix):
    args = _adjust_case(50, dtype, mix)
    y = dops.adjust_logits_rows(*args)
    assert y.dtype == torch.float32
    assert_exact(y.view(torch.int32), _adjust_scalar(*args).view(torch.int32))
    m = _untouched(*args)
    assert m.any() and (~m).any()
    assert torch.equal(y.view(torch.int32)[m], args[0].float().view(torch.int32)[m])
    assert not m[:, 1].all() and m[:, 0].all()  # -0.0 penalised where live, +0.0 never


def _state_update(dev):
    V = 40
    F = dops.PROMPT_FLAG
    state = torch.zeros(4, V, dtype=torch.int32)
    state[1, [3, 7]] = F
    state[2, 5] = F | 2
    state[3, 9] = 4
    before = state.clone()
    state = state.to(dev)
    for ids in ([3, 11, 5, 9], [3, 11, 6, 9], [8, 11, 5, 9]):
        dops.token_state_update(state, [1, 0, 2, -1], torch.tensor(ids, device=dev))
    state = state.cpu()
    want = before.clone()
    want[1, 3] = F | 2
    want[1, 8] = 1
    want[0, 11] = 3
    want[2, 5] = F | 4
    want[2, 6] = 1
    assert_exact(state, want)
    assert int(state[1, 7]) == F and torch.equal(state[3], before[3])  # flags intact, slot -1 row untouched


def test_state_update_cpu():
    _state_update(torch.device("cpu"))


def _check_logprobs(V, dtype, dev, unaligned=False):
    x, ids, ref, order = _logprob_case(V, dtype)
    xd = x.to(dev)
    if unaligned:
        xd = _unaligned(xd)
    chosen, top_ids, top_lp = (t.cpu() for t in dops.logprob_rows(xd, ids.to(dev), N_TOP))
    assert chosen.dtype == torch.float32 and top_ids.dtype == torch.int32 and top_lp.dtype == torch.float32
    assert tuple(top_ids.shape) == (5, 20) and tuple(top_lp.shape) == (5, 20)
    scale = x.float().abs().amax(-1).double()
    for b, n in enumerate(N_TOP):
        if n < 0:
            assert chosen[b] == float("-inf")
        n = max(n, 0)
        assert top_ids[b, :n].tolist() == order[b][:n], (V, b)
        assert (top_ids[b, n:] == -1).all() and (top_lp[b, n:] == float("-inf")).all()
        if N_TOP[b] < 0:
            continue
        print(f"V={V} row {b}: chosen err {abs(chosen[b].double() - ref[b, ids[b]]).item():.3g}, top err "
              f"{(top_lp[b, :n].double() - ref[b, order[b][:n]]).abs().max().item() if n else 0:.3g}, "
              f"scale {scale[b].item():.3g}")
        assert_parity(chosen[b:b + 1], ref[b, ids[b]].view(1), LOGPROB, scale=float(scale[b]), name=f"chosen_lp[{b}]")
        assert_parity(top_lp[b, :n], ref[b, order[b][:n]], LOGPROB, scale=float(scale[b]), name=f"top_lp[{b}]")


@pytest.mark.parametrize("V,dtype", LOGPROB_CASES)
def test_logprob_rows_cpu(V, dtype):
    _check_logprobs(V, dtype, torch.device("cpu"))


@pytest.mark.parametrize("V,dtype", [c for c in LOGPROB_CASES if c[1] == torch.bfloat16])
def test_logprob_cases_contain_ties(V, dtype):
    """The bf16 cases tie inside the top 21, so the lower-id rule decides part of the order."""
    x, _, _, order = _logprob_case(V, dtype)
    ties = sum(int(x[b, o[i]] == x[b, o[i + 1]]) for b, o in enumerate(order) for i in range(20))
    assert ties > 0


def _greedy_case():
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(4, 777, generator=g) * 2).to(torch.bfloat16)
    x[1, [600, 13, 400]] = x[1].max() + 1  # a tied maximum: the lowest id wins
    x[2, [0, 1]] = torch.tensor([-0.0, 0.0], dtype=torch.bfloat16)
    x[2, 2:] = -abs(x[2, 2:]) - 1  # maximum -0.0 == +0.0, a tie: id 0
    return x


def _check_greedy(dev):
    x = _greedy_case().to(dev)
    ids = dops.sample_rows(x, [0.0] * 4, [1.0] * 4, [0] * 4, [1, 2, 3, 4], [0] * 4)
    chosen, top_ids, top_lp = dops.logprob_rows(x, ids, [1, 3, 2, 20])
    assert ids.tolist()[1:3] == [13, 0]
    assert torch.equal(top_ids[:, 0].long().cpu(), ids.cpu())
    assert torch.equal(top_lp[:, 0].contiguous().view(torch.int32), chosen.view(torch.int32))
    assert top_ids[1, :3].tolist() == [13, 400, 600] and top_ids[2, :2].tolist() == [0, 1]


def test_greedy_consistency_cpu():
    _check_greedy(torch.device("cpu"))


def _penalised_sampling_case():
    """One V=1000 row (the recipe of tests/test_sampling.py), the top 3 tokens banned with a
    bias of -100 and a frequency penalty on 10 others; the oracle distribution."""
    V, temp, top_k, top_p = 1000, 0.7, 50, 0.9
    g = torch.Generator().manual_seed(V)
    row = (torch.randn(V, generator=g) * 2.0).to(torch.bfloat16)
    order = row.float().argsort(descending=True)
    banned, counted = order[:3], order[3:13]
    state = torch.zeros(1, V, dtype=torch.int32)
    state[0, counted] = torch.arange(1, 11, dtype=torch.int32)
    bias = torch.zeros(1, V)
    bias[0, banned] = -100.0
    adj = dops.adjust_logits_rows(row.view(1, V), state, [0], [0.0], [0.3], [1.0], bias)[0]
    ref = dops.filter_probs(adj, temp, top_k, top_p)
    return row, state, bias, banned, ref, (temp, top_k, top_p)


def test_penalised_sampling_oracle_bans_the_biased_tokens():
    row, _, _, banned, ref, (temp, top_k, top_p) = _penalised_sampling_case()
    assert (ref[banned] == 0).all() and abs(float(ref.sum()) - 1) < 1e-5
    plain = dops.filter_probs(row.float(), temp, top_k, top_p)
    assert (plain[banned] > 0).all()  # without the bias they carry mass: the case is not vacuous
    assert 0.5 * (plain - ref).abs().sum() > 0.2


def test_neighbour_invariance_cpu():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(4, 300, generator=g) * 2).to(torch.bfloat16)
    state = torch.zeros(2, 300, dtype=torch.int32)
    state[1, :50] = 2
    temps, ps, ks, seeds = [0.0, 0.8, 1.0, 1.2], [1.0, 0.9, 1.0, 0.7], [0, 0, 20, 5], [1, 2, 3, 4]
    for step in range(3):
        want = dops.sample_rows(x, temps, ps, ks, seeds, [step] * 4)
        y = dops.adjust_logits_rows(x, state, [-1, -1, 1, -1], [0.5] * 4, [0.5] * 4, [1.2] * 4)
        got = dops.sample_rows(y, temps, ps, ks, seeds, [step] * 4)
        assert got[[0, 1, 3]].tolist() == want[[0, 1, 3]].tolist()


# --------------------------------------------------------------------------- GPU: the kernels
@pytest.mark.gpu
@pytest.mark.parametrize("V", [50, 777, 1000])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("mix", [0, 1])
def test_adjust_gpu_exact(gpu, V, dtype, mix):
    x, state, slots, pres, freq, rep, bias = _adjust_case(V, dtype, mix)
    want = dops.adjust_logits_rows(x, state, slots, pres, freq, rep, bias)
    m = _untouched(x, state, slots, pres, freq, rep, bias)
    sd, bd = state.to(gpu), (bias.to(gpu) if bias is not None else None)
    for xd in (x.to(gpu), _unaligned(x.to(gpu))):
        y = dops.adjust_logits_rows(xd, sd, slots, pres, freq, rep, bd).cpu()
        assert_exact(y, want, f"adjusted logits V={V}")
        assert_exact(y.view(torch.int32), want.view(torch.int32), "bits (signed zeros)")
        assert torch.equal(y.view(torch.int32)[m], x.float().view(torch.int32)[m])
    if bias is not None:  # no token state: bias only
        y = dops.adjust_logits_rows(x.to(gpu), None, slots, pres, freq, rep, bd).cpu()
        want = dops.adjust_logits_rows(x, None, slots, pres, freq, rep, bias)
        assert_exact(y.view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
def test_adjust_gpu_exact_vocab_128k(gpu):
    V = 128256
    g = torch.Generator().manual_seed(V)
    x = (torch.randn(2, V, generator=g) * 3).to(torch.bfloat16)
    state = (torch.randint(0, 8, (3, V), generator=g) * (torch.rand(3, V, generator=g) < 0.2)).to(torch.int32)
    state |= torch.where(torch.rand(3, V, generator=g) < 0.3, dops.PROMPT_FLAG, 0).to(torch.int32)
    bias = torch.zeros(3, V)
    bias[2, torch.randperm(V, generator=g)[:300]] = torch.randn(300, generator=g) * 50
    args = ([2, 0], [0.4, -0.3], [0.25, 1.1], [1.3, 0.8])
    want = dops.adjust_logits_rows(x, state, *args, bias)
    y = dops.adjust_logits_rows(x.to(gpu), state.to(gpu), *args, bias.to(gpu)).cpu()
    assert_exact(y.view(torch.int32), want.view(torch.int32), "adjusted logits V=128256")


@pytest.mark.gpu
def test_state_update_gpu(gpu):
    _state_update(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("V,dtype", LOGPROB_CASES)
def test_logprob_rows_gpu(gpu, V, dtype):
    _check_logprobs(V, dtype, gpu)
    _check_logprobs(V, dtype, gpu, unaligned=True)


@pytest.mark.gpu
def test_greedy_consistency_gpu(gpu):
    _check_greedy(gpu)


@pytest.mark.gpu
def test_gpu_sampler_frequencies_under_penalties(gpu):
    row, state, bias, banned, ref, (temp, top_k, top_p) = _penalised_sampling_case()
    assert (ref[banned] == 0).all()
    V, n = row.numel(), 20000
    logits = row.to(gpu).unsqueeze(0).expand(n, V).contiguous()
    adj = dops.adjust_logits_rows(logits, state.to(gpu), [0] * n, [0.0] * n, [0.3] * n, [1.0] * n, bias.to(gpu))
    ids = dops.sample_rows(adj, [temp] * n, [top_p] * n, [top_k] * n, [7] * n, list(range(n))).cpu()
    emp = torch.bincount(ids, minlength=V).float() / n
    assert (emp[ref == 0] == 0).all(), "drew a token outside the support (a banned token among them)"
    tv = 0.5 * (emp - ref).abs().sum().item()
    assert tv < 0.04, tv


@pytest.mark.gpu
def test_neighbour_invariance_gpu(gpu):
    """Rows without penalties pushed through the adjusted f32 path (because a batch neighbour
    has penalties) draw what ``sample_rows`` draws from the original bf16 logits."""
    V, B = 128256, 6
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, V, generator=g) * 2).to(torch.bfloat16).to(gpu)
    state = torch.zeros(2, V, dtype=torch.int32, device=gpu)
    state[1, ::3] = 2
    temps, ps = [0.0, 0.7, 1.0, 1.3, 0.9, 0.2], [1.0, 1.0, 0.9, 0.5, 1.0, 0.8]
    ks, seeds = [0, 0, 0, 40, 20, 0], [1, 2, 3, 4, 5, 123456789]
    keep = [0, 1, 2, 3, 5]
    for step in (0, 1, 2):
        want = dops.sample_rows(x, temps, ps, ks, seeds, [step] * B)
        y = dops.adjust_logits_rows(x, state, [-1, -1, -1, -1, 1, -1], [0.5] * B, [0.5] * B, [1.2] * B)
        got = dops.sample_rows(y, temps, ps, ks, seeds, [step] * B)
        assert got[keep].tolist() == want[keep].tolist(), step
    # temperature-only rows (the vocabulary-split kernel) and all-greedy batches take the same route
    for t in ([0.0] * B, [0.7] * B):
        y = dops.adjust_logits_rows(x, None, [-1] * B, [0.0] * B, [0.0] * B, [1.0] * B)
        assert torch.equal(dops.sample_rows(y, t, [1.0] * B, [0] * B, seeds, [4] * B),
                           dops.sample_rows(x, t, [1.0] * B, [0] * B, seeds, [4] * B))


if __name__ == "__main__":
    _measure()
