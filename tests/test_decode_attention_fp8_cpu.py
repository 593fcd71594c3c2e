"""fp8 KV cache for static-cache decode (CPU): the quantisation recipe, the
fp32 reference twins, StaticKVCache/generation flags, and a model-level
error inequality calibrated on the references alone. The helpers here are
shared with tests/test_decode_attention_fp8_gpu.py."""

import copy
import functools
import math

import pytest
import torch

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import GPTModel, StaticKVCache
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_attention, kv_cache_store_fp8
from paddlefleetx_amd.parallel.env import init_dist_env

FP8 = torch.float8_e4m3fn
NAN_CODE = 0x7F


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


# ---------------------------------------------------------------------------
# shared helpers
# ---------------------------------------------------------------------------

def half_ulp_excess(x, codes, scale):
    """max over elements of |deq - x| / bound, bound = (2^-4 |x| + 2^-10
    scale) * (1 + 1e-5): half an e4m3 ulp in the normal range (3 mantissa
    bits) plus half a subnormal step (2^-9) of the scaled row. <= 1 passes.
    Computed in fp64 so the check adds no rounding of its own."""
    x = x.double()
    deq = codes.float().double() * scale.double()[..., None]
    bound = (2.0 ** -4 * x.abs() + 2.0 ** -10 * scale.double()[..., None]) \
        * (1 + 1e-5)
    # an all-zero row has bound 2^-10 and error 0
    return ((deq - x).abs() / bound).max().item()


def finite_codes():
    """All 254 finite e4m3 values (fp32), NaN codes 0x7F/0xFF left out."""
    c = torch.arange(256, dtype=torch.uint8)
    c = c[(c & 0x7F) != NAN_CODE]
    return c.view(FP8).float()


def representable_rows(shape, seed):
    """bf16 rows [..., D] that the recipe stores without rounding: entries
    c * 2^k for e4m3 values c, one entry of every row is +-448, so
    amax = 448 * 2^k, scale = 2^k and inv = 2^-k exactly. k varies by row."""
    g = torch.Generator().manual_seed(seed)
    vals = finite_codes()
    idx = torch.randint(0, vals.numel(), shape, generator=g)
    x = vals[idx]
    top = torch.randint(0, shape[-1], shape[:-1], generator=g)
    sign = torch.randint(0, 2, shape[:-1], generator=g).float() * 2 - 1
    x.scatter_(-1, top[..., None], (448.0 * sign)[..., None])
    k = torch.randint(-6, 3, shape[:-1], generator=g).float()
    x = x * torch.exp2(k)[..., None]
    assert torch.equal(x.to(torch.bfloat16).float(), x)
    return x.to(torch.bfloat16)


def tiny_gpt_pair():
    """(bf16, fp32) tiny GPTs on the CPU with identical (bf16-rounded)
    weights: hidden 256, 2 layers, 2 heads, D = 128."""
    kw = dict(vocab_size=512, hidden_size=256, num_layers=2,
              num_attention_heads=2, max_position_embeddings=64,
              hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(11)
    gpt32 = GPTModel(fused_attn=False, dtype=torch.float32, **kw).eval()
    # private generator: the weights must not depend on what ran before
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for p in gpt32.parameters():
            if p.dim() > 1:
                p.normal_(0.0, 0.02, generator=g)
            p.copy_(p.to(torch.bfloat16).float())
    gpt16 = GPTModel(dtype=torch.bfloat16, **kw).eval()
    gpt16.load_state_dict({n: t.to(torch.bfloat16)
                           for n, t in gpt32.state_dict().items()})
    return gpt16, gpt32


P_LEN, N_DEC = 16, 6


def teacher_forced_error(gpt, want, ids, pos, cache):
    """max |logits - want| over prefill P_LEN + N_DEC decode steps of `gpt`
    run with `cache` (None: tuple cache, else a StaticKVCache)."""
    gen = GPTForGeneration(gpt, {})
    dev = next(gpt.parameters()).device
    ids, pos = ids.to(dev), pos.to(dev)
    err = 0.0
    with torch.no_grad():
        lg, cache = gen._logits(ids[:, :P_LEN], pos[:, :P_LEN], cache)
        err = max(err, (lg.cpu() - want[:, P_LEN - 1]).abs().max().item())
        for t in range(P_LEN, P_LEN + N_DEC):
            lg, cache = gen._logits(ids[:, t:t + 1], pos[:, t:t + 1], cache)
            err = max(err, (lg.cpu() - want[:, t]).abs().max().item())
    return err


def fp8_cache(dev=None):
    return StaticKVCache(2, 2, 2, P_LEN + N_DEC, 128, device=dev,
                         kv_dtype="fp8")


@functools.lru_cache(maxsize=None)
def model_reference_errors():
    """(gpt16, ids, pos, want, e_old, e_sim): everything the model-level
    inequality needs that comes from references alone. e_old: bf16 model,
    tuple cache; e_sim: fp32 model, fp8 twin cache; both against the fp32
    model's logits `want`."""
    gpt16, gpt32 = tiny_gpt_pair()
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 512, (2, P_LEN + N_DEC), generator=g)
    pos = torch.arange(P_LEN + N_DEC).unsqueeze(0).expand(2, -1)
    with torch.no_grad():
        hid = gpt32(ids, pos)
        want = hid @ gpt32.embeddings.word_embeddings.weight.t()  # [2,S,V]
    e_old = teacher_forced_error(gpt16, want, ids, pos, None)
    e_sim = teacher_forced_error(gpt32, want, ids, pos, fp8_cache())
    return gpt16, ids, pos, want, e_old, e_sim


# ---------------------------------------------------------------------------
# 1. recipe
# ---------------------------------------------------------------------------

def test_recipe_bound_and_exact_roundtrip():
    g = torch.Generator().manual_seed(0)
    rows = []
    for mag in (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2):
        rows.append(torch.randn(512, 128, generator=g) * mag)
    # rows with one large outlier use the subnormal end of the code range
    out = torch.randn(64, 128, generator=g)
    out[:, 7] = 300.0
    rows += [out, torch.zeros(1, 128)]
    x = torch.cat(rows).to(torch.bfloat16)
    codes, scale = ref.quantize_kv_rows(x)
    assert codes.dtype == FP8 and codes.shape == x.shape
    assert scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
    deq = ref.dequantize_kv_rows(codes, scale)
    assert deq.dtype == torch.float32
    assert not torch.isnan(codes.float()).any() and torch.isfinite(deq).all()
    assert (codes.view(torch.uint8) & 0x7F).max().item() == 0x7E  # 448
    ratio = half_ulp_excess(x.float(), codes, scale)
    print(f"worst |deq-x|/bound = {ratio:.4f}")
    assert ratio <= 1.0
    # the all-zero row: scale 1, codes 0
    assert scale[-1].item() == 1.0
    assert (codes[-1].view(torch.uint8) == 0).all()

    # exactly representable after scaling: bit-exact round trip
    xr = representable_rows((64, 128), seed=1)
    cr, sr = ref.quantize_kv_rows(xr)
    assert torch.equal(ref.dequantize_kv_rows(cr, sr), xr.float())
    # every finite code in one row, amax = 448 * 2^-3
    allc = (finite_codes() * 0.125)[None]
    ca, sa = ref.quantize_kv_rows(allc)
    assert sa.item() == 0.125
    assert torch.equal(ca.float(), finite_codes()[None])


# ---------------------------------------------------------------------------
# 2. twins
# ---------------------------------------------------------------------------

def _poisoned_fp8_cache(data, lens):
    """Quantise fp32 `data` [B,h,Smax,D]; positions >= lens[b] get NaN codes
    and NaN scales."""
    codes, scale = ref.quantize_kv_rows(data)
    codes, scale = codes.clone(), scale.clone()
    for b, L in enumerate(lens):
        codes.view(torch.uint8)[b, :, L:] = NAN_CODE
        scale[b, :, L:] = float("nan")
    return codes, scale


def test_twin_equals_dequantised_cache_decode():
    torch.manual_seed(2)
    B, h, D, Smax = 4, 2, 64, 40
    lens = [0, 1, 17, 39]
    scale = 1.0 / math.sqrt(D)
    qkv = torch.randn(B, 1, h, 3, D)
    kc, ks = _poisoned_fp8_cache(torch.randn(B, h, Smax, D) * 3.0, lens)
    vc, vs = _poisoned_fp8_cache(torch.randn(B, h, Smax, D), lens)
    kc0, ks0, vc0, vs0 = kc.clone(), ks.clone(), vc.clone(), vs.clone()
    seq_lens = torch.tensor(lens, dtype=torch.int32)

    # fp32 caches holding the dequantised values; ref.decode_attention
    # appends the new token's fp32 K/V there, i.e. keeps it unquantised
    want = ref.decode_attention(qkv, ref.dequantize_kv_rows(kc, ks),
                                ref.dequantize_kv_rows(vc, vs), seq_lens,
                                scale)
    out = decode_attention(qkv, kc, vc, seq_lens, scale=scale,
                           k_scale=ks, v_scale=vs)
    assert out.shape == (B, 1, h * D) and out.dtype == qkv.dtype
    assert torch.isfinite(out).all()
    assert torch.allclose(out, want, atol=1e-5, rtol=0)
    assert torch.equal(seq_lens, torch.tensor(lens, dtype=torch.int32))

    for which, (c, s, c0, s0) in ((1, (kc, ks, kc0, ks0)),
                                  (2, (vc, vs, vc0, vs0))):
        exp_c, exp_s = c0.clone(), s0.clone()
        for b, L in enumerate(lens):
            qc, qs = ref.quantize_kv_rows(qkv[b, 0, :, which])
            exp_c[b, :, L] = qc
            exp_s[b, :, L] = qs
        assert torch.equal(c.view(torch.uint8), exp_c.view(torch.uint8))
        assert torch.equal(s.view(torch.int32), exp_s.view(torch.int32))

    with pytest.raises(AssertionError, match="k_scale"):
        decode_attention(qkv, kc, vc, seq_lens)


def test_kv_store_twin():
    torch.manual_seed(3)
    B, S, h, D, Smax = 2, 5, 2, 64, 8
    qkv = torch.randn(B, S, h, 3, D)
    kc = torch.full((B, h, Smax, D), NAN_CODE, dtype=torch.uint8).view(FP8)
    vc = kc.clone()
    ks = torch.full((B, h, Smax), float("nan"))
    vs = ks.clone()
    kv_cache_store_fp8(qkv, kc, vc, ks, vs)
    for c, s, which in ((kc, ks, 1), (vc, vs, 2)):
        qc, qs = ref.quantize_kv_rows(qkv[:, :, :, which].transpose(1, 2))
        assert torch.equal(c[:, :, :S].view(torch.uint8), qc.view(torch.uint8))
        assert torch.equal(s[:, :, :S], qs)
        assert (c[:, :, S:].view(torch.uint8) == NAN_CODE).all()
        assert torch.isnan(s[:, :, S:]).all()
    with pytest.raises(AssertionError, match="Smax"):
        kv_cache_store_fp8(torch.randn(B, Smax + 1, h, 3, D), kc, vc, ks, vs)


# ---------------------------------------------------------------------------
# 3. flags and footprint
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 128])
def test_static_cache_fp8_shapes_and_footprint(D):
    L, B, h, Smax = 3, 2, 4, 24
    c8 = StaticKVCache(L, B, h, Smax, D, dtype=torch.bfloat16, kv_dtype="fp8")
    assert c8.kv_dtype == "fp8" and len(c8) == L
    for i in range(L):
        slot = c8[i]
        assert slot.fp8
        for t in (slot.k, slot.v):
            assert t.dtype == FP8 and t.shape == (B, h, Smax, D)
        for t in (slot.k_scale, slot.v_scale):
            assert t.dtype == torch.float32 and t.shape == (B, h, Smax)
    c16 = StaticKVCache(L, B, h, Smax, D, dtype=torch.bfloat16)
    assert c16.nbytes == 2 * L * B * h * Smax * D * 2
    assert c8.nbytes * 2 * D == c16.nbytes * (D + 4)


def test_defaults_unchanged_and_flag_errors():
    for kv_dtype in (None, "bf16"):
        c = StaticKVCache(2, 1, 2, 8, 16, dtype=torch.bfloat16,
                          kv_dtype=kv_dtype)
        assert c.kv_dtype == "bf16" and c.k_scale is None \
            and c.v_scale is None
        slot = c[1]
        assert not slot.fp8 and slot.k_scale is None and slot.v_scale is None
        assert slot.k.dtype == torch.bfloat16 and slot.k.shape == (1, 2, 8, 16)
    with pytest.raises(AssertionError, match="kv_dtype"):
        StaticKVCache(2, 1, 2, 8, 16, kv_dtype="int8")

    gpt = GPTModel(vocab_size=128, hidden_size=64, num_layers=2,
                   num_attention_heads=4, max_position_embeddings=64,
                   hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                   fused_attn=False).eval()
    with pytest.raises(ValueError, match="static_kv_cache"):
        GPTForGeneration(gpt, {"kv_cache_dtype": "fp8"})
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        GPTForGeneration(gpt, {"kv_cache_dtype": "fp4",
                               "static_kv_cache": True})
    gen = GPTForGeneration(gpt, {"static_kv_cache": True})
    assert gen.kv_cache_dtype == "bf16"
    cache = gen._new_static_cache(2, 8, torch.device("cpu"))
    assert cache.kv_dtype == "bf16" and cache.k[0].dtype == torch.float32
    gen8 = GPTForGeneration(gpt, {"static_kv_cache": True,
                                  "kv_cache_dtype": "fp8",
                                  "max_dec_len": 4,
                                  "decoding_strategy": "greedy_search",
                                  "eos_token_id": 127})
    assert gen8._new_static_cache(2, 8, torch.device("cpu")).kv_dtype == "fp8"
    ids = torch.randint(0, 127, (2, 5))
    out = gen8(ids)
    assert out.shape == (2, 4) and (out >= 0).all() and (out < 128).all()


# ---------------------------------------------------------------------------
# 4. model level
# ---------------------------------------------------------------------------

def test_model_fp8_cache_error_inequality():
    """Teacher-forced prefill 16 + decode 6 against the fp32 model. e_sim
    isolates what quantising the cache costs (fp32 model, fp8 twin cache),
    e_old what bf16 costs (bf16 model, tuple cache). A bf16 model over an
    fp8 cache may err by 1.5 * e_sim (the bf16 and fp32 models round to
    different codes) plus the project's 2 * e_old rule for a bf16 path."""
    gpt16, ids, pos, want, e_old, e_sim = model_reference_errors()
    cache = fp8_cache()
    e_fp8 = teacher_forced_error(copy.deepcopy(gpt16), want, ids, pos, cache)
    print(f"e_old={e_old:.5f} e_sim={e_sim:.5f} e_fp8={e_fp8:.5f} "
          f"bound={1.5 * e_sim + 2.0 * e_old:.5f}")
    assert cache.max_len == P_LEN + N_DEC
    assert cache.lens.tolist() == [P_LEN + N_DEC] * 2
    assert e_old > 0.0 and e_sim > 0.0
    assert e_fp8 <= 1.5 * e_sim + 2.0 * e_old, (e_fp8, e_sim, e_old)
