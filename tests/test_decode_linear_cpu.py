"""decode_linear without a GPU: the fp32 twin against float64, the op's
library fallback, the Generation flag and the fused decoder-layer sequence
on a tiny fp32 GPT (flag on against flag off)."""

import pytest
import torch

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import GPTModel
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_linear
from paddlefleetx_amd.parallel.env import init_dist_env

F64 = torch.float64
# (bias, activation, residual)
EPILOGUES = [(b, a, r) for b in (False, True) for a in (None, "gelu")
             for r in (False, True)]


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


def _inputs(M, N, K, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) * 0.1).to(dtype)
    b = torch.randn(N, generator=g).to(dtype)
    r = torch.randn(M, N, generator=g).to(dtype)
    return x, w, b, r


def _f64(x, w, b, r, act):
    """(reference, magnitude sum S) in float64 from the given inputs."""
    y = x.to(F64) @ w.to(F64).t()
    s = x.to(F64).abs() @ w.to(F64).abs().t()
    if b is not None:
        y = y + b.to(F64)
        s = s + b.to(F64).abs()
    if act == "gelu":
        y = 0.5 * y * (1.0 + torch.tanh(
            0.7978845608028654 * (y + 0.044715 * y ** 3)))
    if r is not None:
        y = y + r.to(F64)
        s = s + r.to(F64).abs()
    return y, s


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("bias,act,res", EPILOGUES)
def test_twin_against_float64(dtype, bias, act, res):
    M, N, K = 5, 24, 96
    x, w, b, r = _inputs(M, N, K, dtype)
    b = b if bias else None
    r = r if res else None
    got = ref.decode_linear(x, w, b, r, act)
    assert got.dtype == dtype and got.shape == (M, N)
    want, s = _f64(x, w, b, r, act)
    # one rounding to the output format + an fp32 sum of K products and the
    # epilogue terms (eps32 per operation, gelu included: about 10 more)
    eps_out = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -24
    bound = eps_out * want.abs() + (K + 16) * 2.0 ** -24 * s + 1e-30
    err = (got.to(F64) - want).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


def test_twin_flattens_nothing_and_checks_activation():
    x, w, b, r = _inputs(2, 8, 32, torch.float32)
    assert torch.equal(ref.decode_linear(x, w, b, r, "none"),
                       ref.decode_linear(x, w, b, r, None))
    with pytest.raises(AssertionError):
        ref.decode_linear(x, w, b, r, "relu")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("bias,act,res", EPILOGUES)
def test_op_m17_falls_back_and_agrees_with_twin(dtype, bias, act, res):
    M, N, K = 17, 24, 96
    x, w, b, r = _inputs(M, N, K, dtype, seed=1)
    b = b if bias else None
    r = r if res else None
    got = decode_linear(x, w, b, r, act)
    want = ref.decode_linear(x, w, b, r, act)
    assert got.dtype == dtype and got.shape == want.shape
    # the fallback rounds the matmul to the dtype before the epilogue: one
    # more rounding than the twin, each of half an ulp of a term <= S
    _, s = _f64(x, w, b, r, act)
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -24
    bound = 2 * eps * s + (K + 16) * 2.0 ** -23 * s
    err = (got.to(F64) - want.to(F64)).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


def test_op_flattens_leading_dims_and_allows_grad_tensors():
    x, w, b, r = _inputs(6, 16, 32, torch.float32, seed=2)
    y3 = decode_linear(x.view(2, 3, 32), w, b, r.view(2, 3, 16), "gelu")
    assert y3.shape == (2, 3, 16)
    assert torch.equal(y3.view(6, 16), decode_linear(x, w, b, r, "gelu"))
    wg = w.clone().requires_grad_(True)
    y = decode_linear(x, wg, b)  # never raises; library ops carry the graph
    assert y.requires_grad
    with pytest.raises(AssertionError):
        decode_linear(x, w, activation="relu")


def test_generation_flag_needs_static_cache():
    gpt = _tiny_gpt()
    with pytest.raises(ValueError, match="fused_decode_linear"):
        GPTForGeneration(gpt, {"fused_decode_linear": True})
    with pytest.raises(ValueError, match="fused_decode_linear"):
        GPTForGeneration(gpt, {"fused_decode_linear": True,
                               "static_kv_cache": False})
    on = GPTForGeneration(gpt, {"fused_decode_linear": True,
                                "static_kv_cache": True})
    off = GPTForGeneration(gpt, {"static_kv_cache": True})
    assert on.fused_decode_linear and not off.fused_decode_linear
    assert on._new_static_cache(1, 4, "cpu").fused_decode_linear
    assert not off._new_static_cache(1, 4, "cpu").fused_decode_linear


def _tiny_gpt():
    torch.manual_seed(11)
    gpt = GPTModel(vocab_size=512, hidden_size=128, num_layers=2,
                   num_attention_heads=2, max_position_embeddings=64,
                   hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                   fused_attn=False).eval()
    # biases start at zero: make every epilogue term count
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for p in gpt.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
    return gpt


def _one_step(gen, ids, tok):
    """Prefill ids, then one decode step on the forced token: its hidden
    state (after final_ln) and the cache."""
    B, P = ids.shape
    cache = gen._new_static_cache(B, P + 2, ids.device)
    pos = torch.arange(P).unsqueeze(0).expand(B, -1)
    with torch.no_grad():
        gen.gpt(ids, pos, caches=cache, use_cache=True)
        hidden, _ = gen.gpt(tok, cache.lens.long().unsqueeze(1), caches=cache,
                            use_cache=True)
    return hidden, cache


def test_fused_layer_sequence_matches_existing_path_fp32(monkeypatch):
    gpt = _tiny_gpt()
    cfg = {"static_kv_cache": True, "max_dec_len": 2}
    gen_off = GPTForGeneration(gpt, cfg)
    gen_on = GPTForGeneration(gpt, dict(cfg, fused_decode_linear=True))
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 511, (3, 7), generator=g)
    tok = torch.randint(0, 511, (3, 1), generator=g)

    calls = []
    from paddlefleetx_amd.models.gpt import model as gpt_model
    orig = gpt_model.decode_linear

    def counting(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    monkeypatch.setattr(gpt_model, "decode_linear", counting)
    h_off, c_off = _one_step(gen_off, ids, tok)
    assert calls == []  # flag off: the existing path, untouched
    h_on, c_on = _one_step(gen_on, ids, tok)
    assert len(calls) == 4 * len(gpt.layers)  # decode step only, 4 per layer
    assert h_on.shape == h_off.shape == (3, 1, 128)
    assert torch.allclose(h_on, h_off, rtol=1e-5, atol=1e-5), \
        float((h_on - h_off).abs().max())
    assert c_on.lens.tolist() == c_off.lens.tolist() == [8, 8, 8]
    for a, b in zip(c_on.k + c_on.v, c_off.k + c_off.v):
        assert torch.allclose(a[:, :, :8], b[:, :, :8], rtol=1e-5, atol=1e-5)


def test_fused_sampling_loop_with_flag_runs_on_cpu():
    """The whole fused-sampling loop (decode_linear logits included) through
    the fallback: greedy ids equal the flag-off run on a model whose top-2
    gaps are far above fp32 noise."""
    gpt = _tiny_gpt()
    cfg = dict(static_kv_cache=True, fused_sampling=True, max_dec_len=4,
               min_dec_len=4, decoding_strategy="greedy_search",
               eos_token_id=511)
    ids = torch.randint(0, 511, (2, 5),
                        generator=torch.Generator().manual_seed(9))
    out_off = GPTForGeneration(gpt, cfg)(ids)
    out_on = GPTForGeneration(gpt, dict(cfg, fused_decode_linear=True))(ids)
    assert out_on.shape == (2, 4)
    assert torch.equal(out_on, out_off)
