"""Shared-prompt decode attention on the CPU: the fp32 twin against
ref.decode_attention on the expanded caches, the shared-prompt StaticKVCache
through GPTForGeneration, and the config errors."""

import math

import pytest
import torch

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import GPTModel, StaticKVCache
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_attention_shared
from paddlefleetx_amd.parallel.env import init_dist_env

SHARED_CFG = {"max_dec_len": 6, "min_dec_len": 6, "eos_token_id": 127,
              "decoding_strategy": "sampling", "num_return_sequences": 3,
              "static_kv_cache": True, "fused_sampling": True,
              "shared_prompt_cache": True}


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


def tiny_gpt():
    torch.manual_seed(0)
    return GPTModel(vocab_size=128, hidden_size=64, num_layers=2,
                    num_attention_heads=4, max_position_embeddings=64,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                    fused_attn=False).eval()


@pytest.mark.parametrize("G", [1, 2, 5])
def test_twin_equals_reference_on_expanded_caches(G):
    torch.manual_seed(G)
    P, h, D, Lcap, Scap = 3, 2, 64, 40, 9
    plens, B = [0, 17, 40], 3 * G
    slens = [(0, 1, 7)[b % 3] for b in range(B)]
    scale = 1.0 / math.sqrt(D)
    qkv = torch.randn(B, 1, h, 3, D)
    kp, vp = torch.randn(2, P, h, Lcap, D).unbind(0)
    kc, vc = torch.randn(2, B, h, Scap, D).unbind(0)
    kp, vp, kc, vc = (t.contiguous() for t in (kp, vp, kc, vc))
    # what decode_attention sees when every row carries its own prompt copy
    ke = torch.full((B, h, Lcap + Scap, D), float("nan"))
    ve = torch.full((B, h, Lcap + Scap, D), float("nan"))
    for b in range(B):
        Lp, s = plens[b // G], slens[b]
        ke[b, :, :Lp + s] = torch.cat((kp[b // G, :, :Lp], kc[b, :, :s]), 1)
        ve[b, :, :Lp + s] = torch.cat((vp[b // G, :, :Lp], vc[b, :, :s]), 1)
        for t, tail in ((kc, s), (vc, s)):
            t[b, :, tail:] = float("nan")
    for p, Lp in enumerate(plens):
        kp[p, :, Lp:] = float("nan")
        vp[p, :, Lp:] = float("nan")
    total = torch.tensor([plens[b // G] + slens[b] for b in range(B)],
                         dtype=torch.int32)
    want = ref.decode_attention(qkv, ke, ve, total, scale)
    kc0 = kc.clone()
    got = decode_attention_shared(
        qkv, kp, vp, torch.tensor(plens, dtype=torch.int32), kc, vc, total, G,
        scale=scale)
    # both sides sum n = Lcap + Scap fp32 terms per channel (|term| <= vmax
    # after the softmax weights) on scores that are D-term fp32 dot products
    # of size <= sabs: |d out| <= 2^-24 * (n + 2 * D * sabs) * vmax each
    n, vmax = Lcap + Scap, torch.nan_to_num(ve).abs().max().item()
    sabs = torch.einsum("bhd,bhsd->bhs", qkv[:, 0, :, 0].abs(),
                        torch.nan_to_num(ke).abs()).max().item() * scale
    tol = 2 * 2.0 ** -24 * (n + 2 * D * sabs) * vmax
    err = (got - want).abs().max().item()
    print(f"G={G} err={err:.3e} tol={tol:.3e}")
    assert got.shape == (B, 1, h * D) and err <= tol
    for b in range(B):  # appended at the row's own length, rest untouched
        assert torch.equal(kc[b, :, slens[b]], qkv[b, 0, :, 1])
        keep = torch.arange(Scap) != slens[b]
        assert torch.equal(kc[b][:, keep].view(torch.int32),
                           kc0[b][:, keep].view(torch.int32))


def test_model_shared_cache_matches_unshared_teacher_forced():
    gpt = tiny_gpt()
    gen = GPTForGeneration(gpt, {"max_dec_len": 5})
    P, G, Lp, N, heads, D = 2, 3, 9, 5, 4, 16
    B = P * G
    torch.manual_seed(7)
    prompt = torch.randint(0, 128, (P, Lp))
    new = torch.randint(0, 128, (B, N))  # every row decodes its own tokens
    pos = torch.arange(Lp + N).unsqueeze(0)
    plain = StaticKVCache(2, B, heads, Lp + N, D, dtype=torch.float32)
    shared = StaticKVCache(2, B, heads, Lp + N, D, dtype=torch.float32,
                           shared_group=G, suffix_len=N)
    with torch.no_grad():
        lu, _ = gen._logits(prompt.repeat_interleave(G, 0),
                            pos[:, :Lp].expand(B, -1), plain)
        ls, _ = gen._logits(prompt, pos[:, :Lp].expand(P, -1), shared)
        assert torch.allclose(ls.repeat_interleave(G, 0), lu, atol=1e-4,
                              rtol=1e-4)
        assert shared.lens.tolist() == [Lp] * B
        assert shared.prefix_lens.tolist() == [Lp] * P
        for t in range(N):
            p = pos[:, Lp + t:Lp + t + 1].expand(B, -1)
            lu, _ = gen._logits(new[:, t:t + 1], p, plain)
            ls, _ = gen._logits(new[:, t:t + 1], p, shared)
            # fp32 summation noise, the agreement the tuple and the static
            # cache are held to
            assert torch.allclose(ls, lu, atol=1e-4, rtol=1e-4), t
    assert shared.max_len == Lp + N and shared.lens.tolist() == [Lp + N] * B
    for i in range(2):
        assert torch.allclose(shared.k[i], plain.k[i][:, :, Lp:], atol=1e-5)
        assert torch.allclose(shared.k_prefix[i],
                              plain.k[i][::G, :, :Lp], atol=1e-5)
    rows = P * Lp + B * N  # instead of B * (Lp + N)
    assert shared.nbytes == 2 * 2 * rows * heads * D * 4
    assert plain.nbytes == 2 * 2 * B * (Lp + N) * heads * D * 4


def test_generation_shared_prompt_shape_and_grouping():
    gen = GPTForGeneration(tiny_gpt(), dict(SHARED_CFG))
    torch.manual_seed(3)
    ids = torch.randint(0, 127, (2, 5))
    out = gen(ids)
    assert out.shape == (6, 6) and (out >= 0).all() and (out < 128).all()
    torch.manual_seed(3)
    with torch.no_grad():
        out2, st = gen._sample_fused(ids, return_state=True)
    assert out2.shape == (6, 6)
    assert torch.equal(st["ids_buf"][:, :5], ids.repeat_interleave(3, 0))
    assert torch.equal(st["ids_buf"][:, 5:11], out2)
    assert st["cache"].prefix_lens.tolist() == [5, 5]
    assert st["cache"].k_prefix[0].shape[0] == 2
    assert st["cache"].k[0].shape[:3] == (6, 4, 6)


@pytest.mark.parametrize("change,match", [
    ({"static_kv_cache": False, "fused_sampling": False}, "static_kv_cache"),
    ({"fused_sampling": False}, "fused_sampling"),
    ({"decoding_strategy": "greedy_search"}, "decoding_strategy"),
    ({"num_return_sequences": 1}, "num_return_sequences"),
    ({"kv_cache_dtype": "fp8"}, "kv_cache_dtype"),
])
def test_config_errors(change, match):
    with pytest.raises(ValueError, match="shared_prompt_cache.*" + match):
        GPTForGeneration(tiny_gpt(), dict(SHARED_CFG, **change))
