"""fp8 prompt prefix of shared-prompt decode attention on the CPU: the fp32
twin against float64, the StaticKVCache buffers, GPTForGeneration with
shared_prompt_dtype: fp8, and the config errors."""

import math

import pytest
import torch

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import GPTModel, StaticKVCache
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_attention_shared
from paddlefleetx_amd.parallel.env import init_dist_env

CFG = {"max_dec_len": 6, "min_dec_len": 6, "eos_token_id": 127,
       "decoding_strategy": "sampling", "num_return_sequences": 3,
       "static_kv_cache": True, "fused_sampling": True,
       "shared_prompt_cache": True, "shared_prompt_dtype": "fp8"}
F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


def tiny_gpt():
    torch.manual_seed(0)
    return GPTModel(vocab_size=128, hidden_size=64, num_layers=2,
                    num_attention_heads=4, max_position_embeddings=64,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                    fused_attn=False).eval()


@pytest.mark.parametrize("D,G,plens", [(64, 2, (33,)), (128, 5, (0, 17, 40))])
def test_twin_against_float64(D, G, plens):
    """fp32 twin vs float64 over (code * scale) || own tokens || new token.
    Both see the same dequantised values up to one fp32 rounding of
    code * scale; the rest is fp32 summation: n terms of size <= vmax on
    D-term scores of size <= sabs, as in the bf16 twin's test."""
    torch.manual_seed(D + G)
    P, h, Lcap, Scap = len(plens), 2, 40, 9
    B = P * G
    slens = [(0, 1, 7)[b % 3] for b in range(B)]
    qkv = torch.randn(B, 1, h, 3, D)
    kq, ks = ref.quantize_kv_rows(torch.randn(P, h, Lcap, D))
    vq, vs = ref.quantize_kv_rows(torch.randn(P, h, Lcap, D))
    kc, vc = torch.randn(2, B, h, Scap, D).unbind(0)
    kc, vc = kc.contiguous(), vc.contiguous()
    want = torch.empty(B, h, D, dtype=torch.float64)
    kmax = max(ref.dequantize_kv_rows(kq, ks).abs().max().item(),
               kc.abs().max().item(), qkv[:, 0, :, 1].abs().max().item())
    vmax = max(ref.dequantize_kv_rows(vq, vs).abs().max().item(),
               vc.abs().max().item(), qkv[:, 0, :, 2].abs().max().item())
    for b in range(B):
        p, Lp, s = b // G, plens[b // G], slens[b]
        K = torch.cat((kq[p, :, :Lp].double() * ks[p, :, :Lp, None].double(),
                       kc[b, :, :s].double(), qkv[b, 0, :, 1:2].double()), 1)
        V = torch.cat((vq[p, :, :Lp].double() * vs[p, :, :Lp, None].double(),
                       vc[b, :, :s].double(), qkv[b, 0, :, 2:3].double()), 1)
        sc = torch.einsum("hd,hsd->hs", qkv[b, 0, :, 0].double(), K)
        want[b] = torch.einsum("hs,hsd->hd",
                               torch.softmax(sc / math.sqrt(D), -1), V)
        kc[b, :, s:] = float("nan")
        vc[b, :, s:] = float("nan")
    for p, Lp in enumerate(plens):  # NaN codes and NaN scales past the end
        kq.view(torch.uint8)[p, :, Lp:] = 0x7F
        vq.view(torch.uint8)[p, :, Lp:] = 0x7F
        ks[p, :, Lp:] = float("nan")
        vs[p, :, Lp:] = float("nan")
    total = torch.tensor([plens[b // G] + slens[b] for b in range(B)],
                         dtype=torch.int32)
    got = decode_attention_shared(
        qkv, kq, vq, torch.tensor(plens, dtype=torch.int32), kc, vc, total, G,
        k_prefix_scale=ks, v_prefix_scale=vs)
    n = Lcap + Scap
    sabs = qkv[:, 0, :, 0].abs().sum(-1).max().item() * kmax / math.sqrt(D)
    tol = 2 * 2.0 ** -24 * (n + 2 * D * sabs) * vmax
    err = (got.double().view(B, h, D) - want).abs().max().item()
    print(f"D={D} G={G} err={err:.3e} tol={tol:.3e}")
    assert got.shape == (B, 1, h * D) and err <= tol
    for b in range(B):  # the same in-place append into the row's own cache
        assert torch.equal(kc[b, :, slens[b]], qkv[b, 0, :, 1])
        assert torch.equal(vc[b, :, slens[b]], qkv[b, 0, :, 2])


def test_cache_buffers_and_nbytes():
    L, B, G, heads, Smax, D, N = 2, 6, 3, 4, 20, 16, 5
    c = StaticKVCache(L, B, heads, Smax, D, dtype=torch.bfloat16,
                      shared_group=G, suffix_len=N, shared_prefix_dtype="fp8")
    P, Lcap = B // G, Smax - N
    for i in range(L):
        s = c[i]
        assert s.shared and not s.fp8
        assert s.k_prefix.dtype == s.v_prefix.dtype == F8
        assert s.k_prefix.shape == s.v_prefix.shape == (P, heads, Lcap, D)
        assert s.k_prefix_scale.dtype == s.v_prefix_scale.dtype == torch.float32
        assert s.k_prefix_scale.shape == s.v_prefix_scale.shape == \
            (P, heads, Lcap)
        assert s.k.dtype == s.v.dtype == torch.bfloat16
        assert s.k.shape == (B, heads, N, D) and s.k_scale is None
    assert c.nbytes == 2 * L * heads * (P * Lcap * (D + 4) + B * N * D * 2)
    for bad in (dict(shared_group=1, suffix_len=None),
                dict(shared_group=G, suffix_len=N, kv_dtype="fp8")):
        with pytest.raises(AssertionError, match="shared_prefix_dtype|bf16"):
            StaticKVCache(L, B, heads, Smax, D, dtype=torch.bfloat16,
                          shared_prefix_dtype="fp8", **bad)


def test_generation_fp8_prompt_shape_and_grouping():
    gen = GPTForGeneration(tiny_gpt(), dict(CFG))
    torch.manual_seed(3)
    ids = torch.randint(0, 127, (2, 5))
    with torch.no_grad():
        out, st = gen._sample_fused(ids, return_state=True)
    assert out.shape == (6, 6) and (out >= 0).all() and (out < 128).all()
    assert torch.equal(st["ids_buf"][:, :5], ids.repeat_interleave(3, 0))
    assert torch.equal(st["ids_buf"][:, 5:11], out)
    c = st["cache"]
    assert c.prefix_lens.tolist() == [5, 5]
    assert c.k_prefix[0].dtype == F8 and c.k_prefix[0].shape[0] == 2
    assert c.k_prefix_scale[0].shape == c.k_prefix[0].shape[:3]
    assert c.k[0].shape[:3] == (6, 4, 6) and c.k[0].dtype != F8
    # the stored prompt is the quantised K of the prefill
    assert torch.isfinite(c.k_prefix_scale[1][:, :, :5]).all()
    assert torch.isfinite(c.k_prefix[1][:, :, :5].float()).all()


@pytest.mark.parametrize("change,match", [
    ({"shared_prompt_dtype": "int8"}, "must be 'bf16' or 'fp8'"),
    ({"shared_prompt_cache": False}, "needs shared_prompt_cache"),
])
def test_config_errors(change, match):
    with pytest.raises(ValueError, match="shared_prompt_dtype.*" + match):
        GPTForGeneration(tiny_gpt(), dict(CFG, **change))
