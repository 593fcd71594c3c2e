"""CPU: the fp32 twin of the fused sampler (ops.sample_token) and the
fused-sampling generation loop against the eager loop."""

import logging

import pytest
import torch

from paddlefleetx_amd.models.gpt.generation import (GPTForGeneration,
                                                    TopKProcess, TopPProcess)
from paddlefleetx_amd.models.gpt.model import GPTModel
from paddlefleetx_amd.models.gpt.processor import (
    LogitsProcessorList, MinLengthLogitsProcessor,
    RepetitionPenaltyLogitsProcessor)
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import sample_token
from paddlefleetx_amd.parallel.env import init_dist_env

V = 128
EOS = 127


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


@pytest.fixture(scope="module")
def gpt():
    torch.manual_seed(0)
    return GPTModel(vocab_size=V, hidden_size=64, num_layers=2,
                    num_attention_heads=4, max_position_embeddings=64,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                    fused_attn=False).eval()


def _prompts(same_rows=False):
    torch.manual_seed(1)
    ids = torch.randint(1, EOS, (3, 5))
    return ids[:1].expand(3, -1).contiguous() if same_rows else ids


def _both(gpt, cfg, ids, interval):
    base = dict(max_dec_len=10, static_kv_cache=True, **cfg)
    want = GPTForGeneration(gpt, base)(ids)
    got = GPTForGeneration(gpt, dict(base, fused_sampling=True,
                                     finish_check_interval=interval))(ids)
    return want, got


# -- loop equivalence ---------------------------------------------------------

@pytest.mark.parametrize("interval", [1, 4, 16])
@pytest.mark.parametrize("cfg", [
    dict(decoding_strategy="greedy_search", eos_token_id=EOS),
    dict(decoding_strategy="greedy_search", eos_token_id=EOS,
         repetition_penalty=1.3, min_dec_len=2),
    dict(top_k=1, eos_token_id=EOS),
    dict(top_k=1, eos_token_id=EOS, temperature=0.7, top_p=0.9,
         repetition_penalty=1.2, min_dec_len=3),
], ids=["greedy", "greedy_pen_minlen", "topk1", "topk1_all_options"])
def test_fused_loop_equals_eager_loop(gpt, cfg, interval):
    want, got = _both(gpt, cfg, _prompts(), interval)
    assert want.shape == (3, 10)
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("interval", [1, 4, 16])
@pytest.mark.parametrize("strategy", ["greedy_search", "sampling"])
@pytest.mark.parametrize("same_rows", [False, True], ids=["one_row", "all_rows"])
def test_fused_loop_early_eos_trim_and_pad(gpt, strategy, same_rows, interval):
    """eos is the token row 0 emits at its third step: with distinct prompts
    some rows finish early and one never does (pad after eos, full length),
    with equal prompts all rows do (the result is trimmed to three tokens)."""
    ids = _prompts(same_rows)
    cfg = dict(decoding_strategy=strategy, top_k=1, repetition_penalty=20.0)
    free, _ = _both(gpt, dict(cfg, eos_token_id=V + 5), ids, 1)
    eos, pad = int(free[0, 2]), 3
    assert eos not in free[0, :2].tolist()
    finishing = [b for b in range(3) if eos in free[b].tolist()]
    want, got = _both(gpt, dict(cfg, eos_token_id=eos, pad_token_id=pad), ids,
                      interval)
    if same_rows:
        assert finishing == [0, 1, 2] and want.shape == (3, 3)
    else:
        assert 0 < len(finishing) < 3 and want.shape == (3, 10)
        for b in finishing:
            j = free[b].tolist().index(eos)
            assert want[b, j] == eos and (want[b, j + 1:] == pad).all()
    assert got.shape == want.shape and torch.equal(got, want)


def test_fused_sampling_is_seed_reproducible(gpt):
    cfg = dict(max_dec_len=8, static_kv_cache=True, fused_sampling=True,
               top_k=20, top_p=0.9, eos_token_id=EOS)
    gen = GPTForGeneration(gpt, cfg)
    ids = _prompts()
    torch.manual_seed(7)
    a = gen(ids)
    torch.manual_seed(7)
    b = gen(ids)
    torch.manual_seed(8)
    c = gen(ids)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    assert (a >= 0).all() and (a < V).all()


def test_option_checks(gpt):
    with pytest.raises(ValueError, match="static_kv_cache"):
        GPTForGeneration(gpt, dict(fused_sampling=True))
    with pytest.raises(ValueError, match="finish_check_interval"):
        GPTForGeneration(gpt, dict(fused_sampling=True, static_kv_cache=True,
                                   finish_check_interval=0))
    gen = GPTForGeneration(gpt, dict(fused_sampling=True, static_kv_cache=True,
                                     max_dec_len=4))
    with pytest.raises(ValueError, match="logits_processors"):
        gen.sample(_prompts(), logits_processors=LogitsProcessorList())
    small = GPTForGeneration(gpt, dict(fused_sampling=True, max_dec_len=4,
                                       static_kv_cache=True,
                                       kv_cache_capacity=6))
    with pytest.raises(ValueError, match="kv_cache_capacity"):
        small(_prompts())


def test_capture_decode_stays_eager_on_cpu(gpt):
    cfg = dict(max_dec_len=6, static_kv_cache=True, fused_sampling=True,
               decoding_strategy="greedy_search", eos_token_id=EOS)
    want = GPTForGeneration(gpt, cfg)(_prompts())
    gen = GPTForGeneration(gpt, dict(cfg, capture_decode=True))
    said = []

    class _Grab(logging.Handler):
        def emit(self, record):
            said.append(record.getMessage())

    lg, grab = logging.getLogger("paddlefleetx_amd"), _Grab()
    lg.addHandler(grab)
    try:
        got1, got2 = gen(_prompts()), gen(_prompts())
    finally:
        lg.removeHandler(grab)
    assert torch.equal(got1, want) and torch.equal(got2, want)
    assert gen._graph_state is None
    assert len([m for m in said if "capture_decode" in m]) == 1  # once


def test_fixed_capacity_does_not_change_tokens(gpt):
    cfg = dict(max_dec_len=6, static_kv_cache=True, fused_sampling=True,
               top_k=8, eos_token_id=EOS)
    torch.manual_seed(5)
    a = GPTForGeneration(gpt, cfg)(_prompts())
    torch.manual_seed(5)
    b = GPTForGeneration(gpt, dict(cfg, kv_cache_capacity=40))(_prompts())
    assert torch.equal(a, b)


# -- the twin -------------------------------------------------------------------

def _state(B, T, lens, prompt_hi=V):
    torch.manual_seed(2)
    ids_buf = torch.randint(0, prompt_hi, (B, T))
    return (ids_buf, torch.tensor(lens, dtype=torch.int32),
            torch.ones(B, dtype=torch.bool), torch.rand(B, T),
            torch.full((B, 1), -1, dtype=torch.long))


@pytest.mark.parametrize("top_k,top_p,temp,pen", [
    (0, 1.0, 1.0, 1.0), (8, 1.0, 1.0, 1.0), (0, 0.9, 1.0, 1.0),
    (0, 0.5, 0.7, 1.3), (40, 0.9, 0.7, 1.3), (1, 0.9, 1.0, 1.3),
    (V, 1e-6, 1.0, 1.0),
])
def test_twin_filter_equals_processor_chain(top_k, top_p, temp, pen):
    """Kept sets of the twin == MinLength + RepetitionPenalty + TopKProcess +
    TopPProcess on tie-free inputs (randn logits have no ties).

    One corner is not TopPProcess's: when the largest probability alone
    exceeds top_p, the shortest prefix whose mass exceeds top_p is that one
    token (sample_token, and the reference implementation this project was
    modelled on), while TopPProcess here also clears the removal flag of
    the first token BEFORE its shift and so keeps the runner-up as well.
    There the twin's set must be TopPProcess's minus exactly the runner-up.
    """
    B, T = 4, 12
    lens = [3, 7, 9, 12]
    min_length = 8  # rows 0, 1 are below it
    ids_buf, lens_t, _, _, _ = _state(B, T, lens)
    ids_buf[1, 2] = ids_buf[1, 0]  # duplicated history token
    torch.manual_seed(3)
    logits = 3.0 * torch.randn(B, V)
    x, probs, keep = ref.sample_token_filter(
        logits, ids_buf, lens_t, temp, top_k, top_p, pen, min_length, EOS)
    corner_seen = []
    for b in range(B):
        hist = ids_buf[b:b + 1, :lens[b]]
        want = MinLengthLogitsProcessor(min_length, EOS)(hist, logits[b:b + 1])
        if pen != 1.0:
            want = RepetitionPenaltyLogitsProcessor(pen)(hist, want)
        assert torch.equal(x[b:b + 1], want)
        p = torch.softmax(want / temp, dim=-1)
        assert torch.equal(probs[b:b + 1], p)
        assert p.unique().numel() == V  # tie-free
        if top_k > 0:
            p = TopKProcess(p, top_k)
        if top_p < 1.0:
            top2 = torch.topk(p, 2, dim=-1)
            alone = bool(top2.values[0, 0] > top_p)
            p = TopPProcess(p, top_p)
            if alone:
                assert int((p > 0).sum()) == (2 if top2.values[0, 1] > 0 else 1)
                p[0, top2.indices[0, 1]] = 0.0
                corner_seen.append(b)
        assert torch.equal(keep[b:b + 1], p > 0), (b, keep[b].sum(), (p > 0).sum())
        assert keep[b].any()
        assert bool(keep[b, EOS]) <= (lens[b] >= min_length)
    if top_p == 1e-6:
        assert corner_seen == list(range(B))
    if top_p >= 0.9 and temp == 1.0:
        assert corner_seen == []  # the plain nucleus cases are all exact


def test_twin_top_p_keeps_whole_tie():
    """The one deliberate deviation from the sort: a tie at the boundary is
    kept whole."""
    logits = torch.full((1, 8), -30.0)
    logits[0, [1, 4, 6]] = 0.0  # three tokens of probability ~1/3
    ids_buf, lens, _, _, _ = _state(1, 4, [2])
    _, probs, keep = ref.sample_token_filter(logits, ids_buf, lens, top_p=0.5)
    assert keep[0].nonzero().flatten().tolist() == [1, 4, 6]
    _, _, keep = ref.sample_token_filter(logits, ids_buf, lens, top_p=0.2)
    assert keep[0].nonzero().flatten().tolist() == [1, 4, 6]


def test_twin_even_grid_of_u_is_inverse_cdf():
    """On an even grid of N values of u the pick count of every token is
    within 2 of N * p / kept_mass (exact for an inverse CDF, plus rounding);
    zero-probability and dropped tokens get no pick."""
    N, Vs = 4000, 32
    torch.manual_seed(4)
    row = 2.0 * torch.randn(Vs)
    row[[0, 5, Vs - 1]] = -float("inf")  # zero probability, first and last too
    logits = row.expand(N, Vs).contiguous()
    ids_buf = torch.zeros(N, 2, dtype=torch.long)
    lens = torch.ones(N, dtype=torch.int32)
    u = torch.zeros(N, 2)
    u[:, 1] = torch.arange(N, dtype=torch.float64).div(N).float()
    unfinished = torch.ones(N, dtype=torch.bool)
    nxt = torch.empty(N, 1, dtype=torch.long)
    count, mass = sample_token(logits, ids_buf, lens, unfinished, u, nxt,
                               top_p=0.8, eos_token_id=-1)
    _, probs, keep = ref.sample_token_filter(logits[:1], ids_buf[:1], lens[:1],
                                             top_p=0.8)
    assert 1 < int(count[0]) == int(keep.sum()) < Vs - 3
    picks = torch.bincount(nxt[:, 0], minlength=Vs).double()
    p = torch.where(keep[0], probs[0], torch.zeros(())).double()
    expect = N * p / p.sum()
    assert (picks - expect).abs().max() <= 2.0, (picks, expect)
    assert (picks[~keep[0]] == 0).all()
    assert torch.equal(ids_buf[:, 1], nxt[:, 0])


def test_twin_state_update():
    B, T = 5, 6
    ids_buf, lens, unfinished, u, nxt = _state(B, T, [0, 2, 5, 6, 3])
    unfinished[4] = False  # already finished: gets pad
    before = ids_buf.clone()
    logits = torch.full((B, V), -5.0)
    logits[:, 9] = 5.0
    logits[1, EOS] = 9.0  # row 1 draws eos
    lens_before = lens.clone()
    count, mass = sample_token(logits, ids_buf, lens, unfinished, u, nxt,
                               greedy=True, eos_token_id=EOS, pad_token_id=1)
    assert nxt[:, 0].tolist() == [9, EOS, 9, 9, 1]
    assert unfinished.tolist() == [True, False, True, True, False]
    assert torch.equal(lens, lens_before)
    changed = (ids_buf != before).nonzero().tolist()
    assert all(c == lens_before[r] for r, c in changed)
    for b, L in enumerate(lens_before.tolist()):
        if L < T:
            assert ids_buf[b, L] == nxt[b, 0]
    assert torch.equal(ids_buf[3], before[3])  # full row: nothing written
    assert count.tolist() == [1] * B and count.dtype == torch.int32
    assert mass.dtype == torch.float32


def test_twin_boundary_uniforms_and_zero_probability():
    """u = 0 picks the first kept token, the largest float below 1 the last;
    neither ever a token of zero probability."""
    logits = torch.tensor([[-float("inf"), 0.0, 1.0, -float("inf"), 2.0,
                            -float("inf")]]).repeat(2, 1)
    ids_buf = torch.zeros(2, 1, dtype=torch.long)
    lens = torch.zeros(2, dtype=torch.int32)
    u = torch.tensor([[0.0], [1.0]]).nextafter(torch.tensor(0.0))
    assert u[0, 0] == 0.0 and u[1, 0] < 1.0
    nxt = torch.empty(2, 1, dtype=torch.long)
    sample_token(logits, ids_buf, lens, torch.ones(2, dtype=torch.bool), u,
                 nxt)
    assert nxt[:, 0].tolist() == [1, 4]
