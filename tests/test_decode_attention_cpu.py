"""Decode attention with a preallocated KV cache: reference op, model
equivalence against the tuple cache, generation, default-off (CPU)."""

import math

import pytest
import torch

from paddlefleetx_amd.models.gpt import model as gpt_model
from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import GPTModel, StaticKVCache
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_attention
from paddlefleetx_amd.parallel.env import init_dist_env


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


def tiny_gpt(fused_attn=False, vocab=128, hidden=64, layers=2, heads=4,
             maxpos=64, seed=0):
    torch.manual_seed(seed)
    return GPTModel(vocab_size=vocab, hidden_size=hidden, num_layers=layers,
                    num_attention_heads=heads, max_position_embeddings=maxpos,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                    fused_attn=fused_attn)


def test_reference_matches_naive_dense():
    torch.manual_seed(1)
    B, h, D, Smax = 4, 2, 64, 40
    lens = [0, 1, 17, 39]
    scale = 1.0 / math.sqrt(D)
    qkv = torch.randn(B, 1, h, 3, D)
    k_cache = torch.full((B, h, Smax, D), float("nan"))
    v_cache = torch.full((B, h, Smax, D), float("nan"))
    for b, L in enumerate(lens):
        k_cache[b, :, :L] = torch.randn(h, L, D)
        v_cache[b, :, :L] = torch.randn(h, L, D)
    k0, v0 = k_cache.clone(), v_cache.clone()
    seq_lens = torch.tensor(lens, dtype=torch.int32)

    out = decode_attention(qkv, k_cache, v_cache, seq_lens, scale=scale)
    assert out.shape == (B, 1, h * D)
    assert torch.equal(seq_lens, torch.tensor(lens, dtype=torch.int32))

    for b, L in enumerate(lens):
        for j in range(h):
            q, kn, vn = qkv[b, 0, j, 0], qkv[b, 0, j, 1], qkv[b, 0, j, 2]
            K = torch.cat([k0[b, j, :L], kn[None]], dim=0)
            V = torch.cat([v0[b, j, :L], vn[None]], dim=0)
            p = torch.softmax((K @ q) * scale, dim=0)
            want = p @ V
            got = out[b, 0, j * D:(j + 1) * D]
            assert torch.allclose(got, want, atol=1e-5, rtol=0), (b, j)
        # appended at L, everything else bitwise unchanged (NaN tail included)
        assert torch.equal(k_cache[b, :, L], qkv[b, 0, :, 1])
        assert torch.equal(v_cache[b, :, L], qkv[b, 0, :, 2])
        for new, old in ((k_cache, k0), (v_cache, v0)):
            keep = torch.ones(Smax, dtype=torch.bool)
            keep[L] = False
            assert torch.equal(new[b][:, keep].view(torch.int32),
                               old[b][:, keep].view(torch.int32))
    # default scale is 1/sqrt(D)
    out2 = ref.decode_attention(qkv, k0.clone(), v0.clone(), seq_lens)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("fused_attn", [False, True])
def test_static_cache_matches_tuple_cache_teacher_forced(fused_attn):
    gpt = tiny_gpt(fused_attn=fused_attn).eval()
    gen = GPTForGeneration(gpt, {"max_dec_len": 5})
    B, P, N = 2, 9, 5
    torch.manual_seed(7)
    ids = torch.randint(0, 128, (B, P + N))
    pos = torch.arange(P + N).unsqueeze(0).expand(B, -1)
    heads, D = 4, 16
    with torch.no_grad():
        static = StaticKVCache(2, B, heads, P + N, D, dtype=torch.float32)
        lt, tc = gen._logits(ids[:, :P], pos[:, :P], None)
        ls, sc = gen._logits(ids[:, :P], pos[:, :P], static)
        assert sc is static and static.max_len == P
        assert torch.allclose(ls, lt, atol=1e-4, rtol=1e-4)
        for t in range(P, P + N):
            lt, tc = gen._logits(ids[:, t:t + 1], pos[:, t:t + 1], tc)
            ls, sc = gen._logits(ids[:, t:t + 1], pos[:, t:t + 1], sc)
            assert sc is static
            assert torch.allclose(ls, lt, atol=1e-4, rtol=1e-4), t
    assert static.max_len == P + N
    assert static.lens.tolist() == [P + N] * B
    # the cache holds what the tuple cache grew to
    for i in range(2):
        assert torch.allclose(static.k[i], tc[i][0], atol=1e-5)
        assert torch.allclose(static.v[i], tc[i][1], atol=1e-5)


def _greedy_pair(seed):
    """(generator with the key absent, generator with it on, prompt) over
    ONE model, B=2, prompt 5, 8 new tokens."""
    gpt = tiny_gpt(seed=seed).eval()
    # model init also draws from the per-rank RNG tracker, whose state
    # depends on what ran before; redraw the matrices from a private
    # generator so the ids (and the top-2 gap) do not depend on test order
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in gpt.parameters():
            if p.dim() > 1:
                p.normal_(0.0, 0.02, generator=g)
    cfg = {"max_dec_len": 8, "decoding_strategy": "greedy_search",
           "eos_token_id": 127}
    gen_off = GPTForGeneration(gpt, dict(cfg))
    gen_on = GPTForGeneration(gpt, dict(cfg, static_kv_cache=True))
    torch.manual_seed(seed)
    ids = torch.randint(0, 127, (2, 5))
    return gen_off, gen_on, ids


def test_generation_static_cache_same_ids():
    # seed 0: the smallest top-2 logit gap over all steps is checked below
    # to be far above the 1e-4 agreement of the two paths
    gen_a, gen_b, ids = _greedy_pair(seed=0)
    assert not gen_a.static_kv_cache and gen_b.static_kv_cache
    out_a = gen_a(ids)
    out_b = gen_b(ids)
    assert out_a.shape == (2, 8)
    assert torch.equal(out_a, out_b)
    # margin check: replay the chosen ids and look at the top-2 gap
    full = torch.cat([ids, out_a], dim=1)
    pos = torch.arange(full.shape[1]).unsqueeze(0).expand(2, -1)
    with torch.no_grad():
        hidden = gen_a.gpt(full, pos)
        logits = hidden @ gen_a.gpt.embeddings.word_embeddings.weight.t()
    top2 = logits[:, 4:-1].topk(2, dim=-1).values
    assert (top2[..., 0] - top2[..., 1]).min() > 1e-4


def test_static_cache_off_by_default(monkeypatch):
    made = []
    orig = StaticKVCache.__init__

    def counting(self, *a, **kw):
        made.append(1)
        orig(self, *a, **kw)

    monkeypatch.setattr(gpt_model.StaticKVCache, "__init__", counting)
    gen_off, gen_on, ids = _greedy_pair(seed=0)
    gen_off(ids)
    assert made == []
    gen_on(ids)
    assert made == [1]


def test_static_cache_rejects_misuse():
    gpt = tiny_gpt().eval()
    static = StaticKVCache(2, 1, 4, 5, 16, dtype=torch.float32)
    ids = torch.randint(0, 128, (1, 3))
    with torch.no_grad():
        gpt(ids, caches=static, use_cache=True)
        with pytest.raises(AssertionError, match="empty cache"):
            gpt(ids[:, :2], caches=static, use_cache=True)
        for p in (3, 4):
            gpt(ids[:, :1], torch.tensor([[p]]), caches=static,
                use_cache=True)
        assert static.max_len == 5
        with pytest.raises(AssertionError, match="overflow"):
            gpt(ids[:, :1], torch.tensor([[5]]), caches=static,
                use_cache=True)
    q = torch.randn(1, 1, 4, 3, 16, requires_grad=True)
    with pytest.raises(AssertionError, match="inference-only"):
        decode_attention(q, static.k[0], static.v[0], static.lens)
