"""fp8 weight storage for decode_linear without a GPU: the per-row weight
quantiser, the fp32 twin against float64, the derived effect of
quantisation, the op's fallback, the Generation flag and the fused decoder
layer with codes on a tiny fp32 GPT.

Quantiser bound (KERNELS.md, decode_linear_fp8): v = w * inv lies in
[-448, 448]; e4m3 has 3 stored mantissa bits, so round-to-nearest is within
2^-4 |v| for normal values and within half the subnormal step, 2^-10, below
2^-6. Times scale (and the fp32 roundings of scale, inv and the product,
far below either term):

    |code * scale - w| <= 2^-4 |w| + 2^-10 scale

Twin bound, r in float64 from the same codes, S = (|x| |codes|^T) scale +
|b| + |res|:

    |y - r| <= 2^-8 |r| + (2K + 2) 2^-24 S + 2^-126

(the bound of test_decode_linear_gpu.py with +2 for the scale multiply),
plus the project's fp32 bias-gelu tolerance when GELU is on.
"""

import copy

import pytest
import torch

from test_ops_edges_gpu import FP32_TOL

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import GPTModel
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_linear
from paddlefleetx_amd.parallel.env import init_dist_env

F64, BF16, F32 = torch.float64, torch.bfloat16, torch.float32
FP8 = torch.float8_e4m3fn
BG_TOL = FP32_TOL["bg.y"]  # (rtol, atol) of the fp32 bias-gelu
# (bias, activation, residual)
EPILOGUES = [(b, a, r) for b in (False, True) for a in (None, "gelu")
             for r in (False, True)]


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


def _weights(N=40, K=192, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF16)
    w[3] = 0                     # a zero row
    w[7, 11] = 60 * 0.05         # one 60-sigma outlier
    return w


def _gelu64(y):
    return 0.5 * y * (1.0 + torch.tanh(
        0.7978845608028654 * (y + 0.044715 * y ** 3)))


def test_quantiser_rows():
    w = _weights()
    codes, scale = ref.quantize_weight_rows(w)
    assert codes.dtype == FP8 and codes.shape == w.shape
    assert scale.dtype == F32 and scale.shape == (w.shape[0],)
    assert bool((scale > 0).all())
    cf = codes.float()
    assert bool(torch.isfinite(cf).all())
    assert float(scale[3]) == 1.0 and bool((cf[3] == 0).all())
    # an outlier row costs the other rows nothing: one scale per row
    assert float(scale[7]) == pytest.approx(3.0 / 448, rel=1e-6)
    assert float(scale[6]) < 0.1 * float(scale[7])
    deq = cf.to(F64) * scale.to(F64)[:, None]
    w64 = w.to(F64)
    bound = 2.0 ** -4 * w64.abs() + 2.0 ** -10 * scale.to(F64)[:, None]
    err = (deq - w64).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"\n[decode_linear_fp8] quantiser worst err/bound = {ratio:.3g}",
          end="")
    assert bool((err <= bound).all()), ratio
    # the arithmetic IS quantize_kv_rows
    kc, ks = ref.quantize_kv_rows(w)
    assert torch.equal(scale.view(torch.int32), ks.view(torch.int32))
    assert torch.equal(codes.view(torch.uint8), kc.view(torch.uint8))


def test_every_finite_code_is_a_bf16_value():
    """What the kernel's in-register decode rests on."""
    allc = torch.arange(256, dtype=torch.uint8).view(FP8).float()
    fin = allc[torch.isfinite(allc)]
    assert fin.numel() == 254
    assert torch.equal(fin.to(BF16).float(), fin)
    assert bool((fin.view(torch.int32) & 0xFFFF == 0).all())


def _case(M, N, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) * 0.1).to(dtype)
    b = torch.randn(N, generator=g).to(dtype)
    r = torch.randn(M, N, generator=g).to(dtype)
    codes, scale = ref.quantize_weight_rows(w)
    return x, w, codes, scale, b, r


def _f64(x, codes, scale, b, r, act):
    c64, s64 = codes.float().to(F64), scale.to(F64)
    y = (x.to(F64) @ c64.t()) * s64
    s = (x.to(F64).abs() @ c64.abs().t()) * s64
    if b is not None:
        y = y + b.to(F64)
        s = s + b.to(F64).abs()
    if act == "gelu":
        y = _gelu64(y)
    if r is not None:
        y = y + r.to(F64)
        s = s + r.to(F64).abs()
    return y, s


def _twin_bound(want, s, K, gelu, dtype):
    eps_out = 2.0 ** -8 if dtype == BF16 else 2.0 ** -24
    bound = eps_out * want.abs() + (2 * K + 2) * 2.0 ** -24 * s + 2.0 ** -126
    if gelu:
        bound = bound + BG_TOL[1] + BG_TOL[0] * want.abs()
    return bound


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("bias,act,res", EPILOGUES)
@pytest.mark.parametrize("M,N,K", [(5, 24, 192), (16, 136, 64),
                                   (2, 16, 8192)])
def test_twin_against_float64(M, N, K, dtype, bias, act, res):
    x, _, codes, scale, b, r = _case(M, N, K, dtype, seed=K + M)
    b = b if bias else None
    r = r if res else None
    got = ref.decode_linear_fp8(x, codes, scale, b, r, act)
    assert got.dtype == dtype and got.shape == (M, N)
    want, s = _f64(x, codes, scale, b, r, act)
    bound = _twin_bound(want, s, K, act == "gelu", dtype)
    err = (got.to(F64) - want).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


def test_effect_of_quantisation_is_within_the_derived_bound():
    """|x deq^T - x w^T| <= 2^-4 |x||w|^T + 2^-10 scale_n sum|x|, in float64:
    the per-element quantiser bound summed along k."""
    for (M, N, K) in [(5, 24, 192), (16, 40, 2112)]:
        x, w, codes, scale, _, _ = _case(M, N, K, BF16, seed=7)
        x64, w64, s64 = x.to(F64), w.to(F64), scale.to(F64)
        deq = codes.float().to(F64) * s64[:, None]
        diff = (x64 @ deq.t() - x64 @ w64.t()).abs()
        bound = 2.0 ** -4 * (x64.abs() @ w64.abs().t()) \
            + 2.0 ** -10 * s64[None, :] * x64.abs().sum(-1, keepdim=True)
        assert bool((diff <= bound).all()), float((diff / bound).max())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("bias,act,res", EPILOGUES)
def test_op_on_cpu_equals_twin(dtype, bias, act, res):
    x, _, codes, scale, b, r = _case(6, 24, 192, dtype, seed=1)
    b = b if bias else None
    r = r if res else None
    got = decode_linear(x.view(2, 3, 192), codes, b,
                        r.view(2, 3, 24) if res else None, act,
                        weight_scale=scale)
    want = ref.decode_linear_fp8(x, codes, scale, b, r, act)
    assert got.shape == (2, 3, 24) and got.dtype == dtype
    assert torch.equal(got.view(6, 24), want)


def test_op_needs_scale_with_fp8_and_only_then():
    x, w, codes, scale, b, r = _case(4, 16, 64, F32, seed=2)
    with pytest.raises(ValueError, match="weight_scale"):
        decode_linear(x, codes)
    with pytest.raises(ValueError, match="weight_scale"):
        decode_linear(x, w, weight_scale=scale)
    with pytest.raises(AssertionError):
        decode_linear(x, codes, activation="relu", weight_scale=scale)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_bf16_calls_are_unchanged(dtype):
    """weight_scale=None with an unquantised weight: the expression the op
    computed before the keyword existed, bit for bit."""
    x, w, _, _, b, r = _case(17, 24, 96, dtype, seed=3)
    got = decode_linear(x, w, b, r, "gelu", weight_scale=None)
    yf = torch.nn.functional.linear(x, w).float() + b.float()
    yf = torch.nn.functional.gelu(yf, approximate="tanh") + r.float()
    assert torch.equal(got, yf.to(dtype))
    assert torch.equal(decode_linear(x, w), torch.nn.functional.linear(x, w))


# ---------------------------------------------------------------------------
# config and model
# ---------------------------------------------------------------------------

def _tiny_gpt():
    torch.manual_seed(11)
    gpt = GPTModel(vocab_size=512, hidden_size=128, num_layers=2,
                   num_attention_heads=2, max_position_embeddings=64,
                   hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                   fused_attn=False).eval()
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for p in gpt.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
    return gpt


def _linear_weights(gpt):
    ws = []
    for layer in gpt.layers:
        ws += [layer.attn.qkv.weight, layer.attn.out_proj.weight,
               layer.ffn.up.weight, layer.ffn.down.weight]
    return ws


def _dequantised_copy(gpt):
    """A copy of the model whose four linears per layer hold code * scale.
    The embedding stays: the lookup reads the unquantised table, only the
    logits (not part of the hidden state) read its codes."""
    m = copy.deepcopy(gpt)
    with torch.no_grad():
        for w in _linear_weights(m):
            c, s = ref.quantize_weight_rows(w)
            w.copy_(ref.dequantize_kv_rows(c, s))
    return m


CFG = {"static_kv_cache": True, "max_dec_len": 2, "fused_decode_linear": True}


def test_generation_flag():
    gpt = _tiny_gpt()
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        GPTForGeneration(gpt, {"decode_weight_dtype": "fp8",
                               "static_kv_cache": True})
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        GPTForGeneration(gpt, dict(CFG, decode_weight_dtype="int8"))
    on = GPTForGeneration(gpt, dict(CFG, decode_weight_dtype="fp8"))
    off = GPTForGeneration(gpt, CFG)
    assert on.decode_weight_dtype == "fp8"
    assert off.decode_weight_dtype == "bf16"
    assert GPTForGeneration(gpt, dict(CFG, decode_weight_dtype="bf16")) \
        .decode_weight_dtype == "bf16"
    c_on = on._new_static_cache(1, 4, "cpu")
    assert c_on.weight_codes is on._weight_codes is not None
    assert c_on.fused_decode_linear
    assert off._new_static_cache(1, 4, "cpu").weight_codes is None
    # the codes are no parameters or buffers: checkpoints are unchanged
    assert list(on.state_dict()) == list(off.state_dict())
    assert list(gpt.state_dict()) == list(_tiny_gpt().state_dict())


def _one_step(gen, ids, tok):
    B, P = ids.shape
    cache = gen._new_static_cache(B, P + 2, ids.device)
    pos = torch.arange(P).unsqueeze(0).expand(B, -1)
    with torch.no_grad():
        gen.gpt(ids, pos, caches=cache, use_cache=True)
        hidden, _ = gen.gpt(tok, cache.lens.long().unsqueeze(1), caches=cache,
                            use_cache=True)
    return hidden, cache


def _ids():
    g = torch.Generator().manual_seed(5)
    return (torch.randint(0, 511, (3, 7), generator=g),
            torch.randint(0, 511, (3, 1), generator=g))


def test_fused_layer_with_codes_matches_dequantised_model(monkeypatch):
    gpt = _tiny_gpt()
    gen = GPTForGeneration(gpt, dict(CFG, decode_weight_dtype="fp8"))
    ids, tok = _ids()
    scaled = []
    from paddlefleetx_amd.models.gpt import model as gpt_model
    orig = gpt_model.decode_linear

    def counting(x, weight, *a, **kw):
        scaled.append(kw.get("weight_scale") is not None
                      and weight.dtype == FP8)
        return orig(x, weight, *a, **kw)

    monkeypatch.setattr(gpt_model, "decode_linear", counting)
    h_on, _ = _one_step(gen, ids, tok)
    assert scaled == [True] * (4 * len(gpt.layers))  # decode step only
    # the reference: prefill with the ORIGINAL weights (the prompt is
    # processed unquantised), the decode token with code * scale
    deq = _dequantised_copy(gpt)
    gen_ref = GPTForGeneration(gpt, CFG)
    B, P = ids.shape
    cache = gen_ref._new_static_cache(B, P + 2, "cpu")
    pos = torch.arange(P).unsqueeze(0).expand(B, -1)
    with torch.no_grad():
        gpt(ids, pos, caches=cache, use_cache=True)
        h_ref, _ = deq(tok, cache.lens.long().unsqueeze(1), caches=cache,
                       use_cache=True)
    assert h_on.shape == h_ref.shape == (3, 1, 128)
    # the fp32 tolerance of test_decode_linear_cpu's fused-layer test
    assert torch.allclose(h_on, h_ref, rtol=1e-5, atol=1e-5), \
        float((h_on - h_ref).abs().max())
    # and quantisation did something: not the unquantised model's state
    h_bf, _ = _one_step(gen_ref, ids, tok)
    assert not torch.allclose(h_on, h_bf, rtol=1e-5, atol=1e-5)


def test_logits_take_codes_in_the_fused_sampling_loop(monkeypatch):
    gpt = _tiny_gpt()
    cfg = dict(static_kv_cache=True, fused_sampling=True, max_dec_len=4,
               min_dec_len=4, decoding_strategy="greedy_search",
               eos_token_id=511, fused_decode_linear=True,
               decode_weight_dtype="fp8")
    gen = GPTForGeneration(gpt, cfg)
    scaled = []
    from paddlefleetx_amd.models.gpt import generation as gen_mod
    from paddlefleetx_amd.models.gpt import model as gpt_model
    orig = gpt_model.decode_linear

    def counting(x, weight, *a, **kw):
        scaled.append(kw.get("weight_scale") is not None
                      and weight.dtype == FP8)
        return orig(x, weight, *a, **kw)

    monkeypatch.setattr(gpt_model, "decode_linear", counting)
    monkeypatch.setattr(gen_mod, "decode_linear", counting)
    ids = torch.randint(0, 511, (2, 5),
                        generator=torch.Generator().manual_seed(9))
    out = gen(ids)
    assert out.shape == (2, 4)
    # 3 decode steps: 4 per layer plus the logits, every one with a scale
    assert scaled == [True] * (3 * (4 * len(gpt.layers) + 1))
    # greedy ids of the model whose decode weights are code * scale, the
    # prompt processed with the original ones: what this mode computes
    assert len(gen._weight_codes) == 4 * len(gpt.layers) + 1


def test_in_place_weight_change_gives_fresh_codes_in_the_same_buffers():
    gpt = _tiny_gpt()
    gen = GPTForGeneration(gpt, dict(CFG, decode_weight_dtype="fp8"))
    ids, tok = _ids()
    h1, _ = _one_step(gen, ids, tok)
    w = gpt.layers[0].attn.qkv.weight
    codes, scale = gen._weight_codes.get(w)
    ptrs = (codes.data_ptr(), scale.data_ptr())
    old = codes.view(torch.uint8).clone()
    with torch.no_grad():
        w.mul_(-1.5)
    h2, _ = _one_step(gen, ids, tok)
    codes2, scale2 = gen._weight_codes.get(w)
    assert (codes2.data_ptr(), scale2.data_ptr()) == ptrs  # in place
    assert not torch.equal(codes2.view(torch.uint8), old)
    want_c, want_s = ref.quantize_weight_rows(w.detach())
    assert torch.equal(codes2.view(torch.uint8), want_c.view(torch.uint8))
    assert torch.equal(scale2, want_s)
    assert not torch.allclose(h1, h2)
    # and the step equals a fresh wrapper's on the changed model
    h3, _ = _one_step(
        GPTForGeneration(gpt, dict(CFG, decode_weight_dtype="fp8")), ids, tok)
    assert torch.equal(h2, h3)


def test_float_cast_leaves_codes_alone():
    gpt = _tiny_gpt().to(BF16)
    gen = GPTForGeneration(gpt, dict(CFG, decode_weight_dtype="fp8"))
    gen._refresh_weight_codes()
    w = gpt.layers[1].ffn.down.weight
    codes, scale = gen._weight_codes.get(w)
    before = codes.view(torch.uint8).clone()
    gen.float()
    w = gpt.layers[1].ffn.down.weight
    codes2, scale2 = gen._weight_codes.get(w)
    assert codes2.dtype == FP8 and scale2.dtype == F32
    assert codes2.data_ptr() == codes.data_ptr()
    # bf16 -> fp32 is exact: re-quantising gives the same codes
    assert torch.equal(codes2.view(torch.uint8), before)
