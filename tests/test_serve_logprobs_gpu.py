"""Serving with logprobs and penalties on the GPU: the captured decode graph and the
out-of-graph kernels of csrc/kernels/logits_proc.hip together (tiny model, graphs on)."""
import pytest
import torch

from mxllm.models import Llama, get_config
from mxllm.ops import decode as dops
from mxllm.serve.engine import Engine, SamplingParams

from .test_logits_proc import LOGPROB

pytestmark = pytest.mark.gpu

PROMPTS = [[1, 2, 3, 4, 5], list(range(10, 80)), [7], list(range(300, 320))]
# GPU against CPU logits of the same bf16 weights: the engine-parity tests of tests/test_model_gpu.py
# hold logits to a relative error of 2e-2 (and greedy tokens to "at most one late flip").  A
# log-probability is a logit minus the row's lse, and the lse moves by at most the largest logit
# error, so the bf16 forward's spread on a log-probability is 2 x 2e-2 of the row's largest |logit|.
FORWARD_REL = 2e-2


def _run(eng, prompts, params):
    reqs = [eng.submit(p, sp) for p, sp in zip(prompts, params)]
    while not all(r.done.is_set() for r in reqs):
        eng.step()
    assert all(r.error is None for r in reqs), [r.error for r in reqs]
    return reqs


@pytest.fixture(scope="module")
def models(gpu):
    cfg = get_config("tiny-d128")
    cpu = Llama(cfg, seed=3).eval()
    dev = Llama(cfg, device=gpu, seed=3).eval()
    dev.load_state_dict(cpu.state_dict())
    return cpu, dev


@pytest.fixture(scope="module")
def engine(models, gpu):
    eng = Engine(models[1], max_batch=4, max_seq=512, use_graphs=True)
    assert eng.use_graphs
    return eng


def test_logprobs_and_a_penalised_neighbour_leave_tokens_alone(engine):
    plain = _run(engine, PROMPTS, [SamplingParams(max_new_tokens=10) for _ in PROMPTS])
    assert engine._tok_state is None and engine._tok_bias is None
    params = [SamplingParams(max_new_tokens=10, logprobs=3) for _ in PROMPTS]
    params[2] = SamplingParams(max_new_tokens=10, frequency_penalty=1.5, repetition_penalty=1.3, logit_bias={9: -100})
    got = _run(engine, PROMPTS, params)
    assert len(engine._graphs) >= 1
    for i in (0, 1, 3):
        assert got[i].output == plain[i].output
        assert len(got[i].logprobs) == 10
        for tok, (lp, top) in zip(got[i].output, got[i].logprobs):
            assert len(top) == 3 and top[0] == (tok, lp) and top[0][1] >= top[1][1] >= top[2][1]
    assert got[2].logprobs == [] and 9 not in got[2].output
    assert int((engine._tok_state & dops.COUNT_MASK).sum()) == 10  # only the penalised request is counted


def test_logprobs_match_the_cpu_engine(engine, models, monkeypatch):
    params = lambda: [SamplingParams(max_new_tokens=8, logprobs=3) for _ in PROMPTS]  # noqa: E731
    got = _run(engine, PROMPTS, params())
    scales = []
    real = dops.logprob_rows

    def spy(x, ids, n_top):
        scales.append(x.float().abs().amax(-1).tolist())
        return real(x, ids, n_top)

    monkeypatch.setattr(dops, "logprob_rows", spy)
    want = _run(Engine(models[0], max_batch=4, max_seq=512), PROMPTS, params())
    monkeypatch.undo()
    assert all(len(w.output) == 8 for w in want) and len(scales) == 8  # every step has all four rows
    compared = 0
    for i, (g, w) in enumerate(zip(got, want)):
        # a near-tie in the bf16 logits may send the two engines down different sequences: the
        # log-probabilities are comparable while the tokens agree
        for t, ((lp, _), (lpw, _)) in enumerate(zip(g.logprobs, w.logprobs)):
            if g.output[:t + 1] != w.output[:t + 1]:
                break
            scale = scales[t][i]  # all four requests run the same steps: row i of step t
            bound = LOGPROB[0] * abs(lpw) + (LOGPROB[1] + 2 * FORWARD_REL) * scale
            print(f"request {i} token {t}: gpu {lp:.6f} cpu {lpw:.6f} |diff| {abs(lp - lpw):.3g} bound {bound:.3g}")
            assert abs(lp - lpw) <= bound, (i, t, lp, lpw, bound)
            compared += 1
    assert compared >= 16, compared  # half of the 32 positions at least
    # prompt scoring has no sequence to diverge: every position of every prompt
    cpu_eng = Engine(models[0], max_batch=4, max_seq=512)
    for ids, g, w in zip(PROMPTS, engine.score(PROMPTS, top=1), cpu_eng.score(PROMPTS, top=1)):
        with torch.no_grad():
            scale = models[0](torch.tensor([ids]))[0].float().abs().amax(-1).tolist()
        assert g[0] is None and len(g) == len(ids)
        for t, (a, b) in enumerate(zip(g[1:], w[1:])):
            bound = LOGPROB[0] * abs(b[0]) + (LOGPROB[1] + 2 * FORWARD_REL) * scale[t]
            assert abs(a[0] - b[0]) <= bound, (t, a, b, bound)


def test_slot_reuse_starts_from_clean_counts(engine, monkeypatch):
    """Six requests through four slots: the second tenant of a slot is penalised by its own
    output only, as in the run where it goes first."""
    prompts = PROMPTS + [[11, 12, 13], list(range(40, 60))]
    pen = lambda n: SamplingParams(max_new_tokens=n, frequency_penalty=1.5, presence_penalty=0.5)  # noqa: E731
    first = _run(engine, prompts[4:], [pen(8), pen(8)])
    seen = []
    real = dops.adjust_logits_rows

    def spy(logits, state, slots, *a, **k):
        seen.append((list(slots), (state & dops.COUNT_MASK).sum(1).tolist()))
        return real(logits, state, slots, *a, **k)

    monkeypatch.setattr(dops, "adjust_logits_rows", spy)
    reqs = [engine.submit(p, sp) for p, sp in zip(prompts, [pen(3), pen(4), pen(5), pen(6), pen(8), pen(8)])]
    slot_of = {}
    while not all(r.done.is_set() for r in reqs):
        engine.step()
        for i, r in enumerate(reqs):
            if r.slot >= 0:
                slot_of.setdefault(i, r.slot)
    # the first adjust call that carries only the late requests' slots is their prefill sample
    for i in (4, 5):
        s = slot_of[i]
        call = next(c for c in seen if c[0] == [s] or (set(c[0]) <= {slot_of[4], slot_of[5]} and s in c[0]))
        assert call[1][s] == 0, f"request {i} inherited {call[1][s]} counts in slot {s}"
        agree = sum(int(a == b) for a, b in zip(reqs[i].output, first[i - 4].output))
        assert agree >= len(reqs[i].output) - 1, (reqs[i].output, first[i - 4].output)
    assert {slot_of[4], slot_of[5]} <= {slot_of[0], slot_of[1], slot_of[2], slot_of[3]}  # reused slots
