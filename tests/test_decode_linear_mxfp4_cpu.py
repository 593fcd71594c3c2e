"""CPU: the MXFP4 quantiser and its twin (ops/_reference.py), the op's
fallback and errors, the Generation flag and DecodeWeightCodes("mxfp4").

Quantisation error. With v = w / 2^p and |v| <= 6 (no block clips), the e2m1
grid has spacing 1/2 on [0, 2], 1 on [2, 4] and 2 on [4, 6]: round-to-nearest
is off by at most 1/4 where |v| <= 2 and by at most |v| / 4 above, so
|deq - w| <= 1/4 max(|w|, 2^p) for every element.
"""

import pytest
import torch

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import DecodeWeightCodes, GPTModel
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_linear

F32, F64, U8 = torch.float32, torch.float64, torch.uint8


def _weight(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.rand(N, 1, generator=g) * 4
    w[1, 32:64] = 0.0                  # a zero block
    w[2, :32] *= 2.0 ** -140           # scale byte clamped at 2
    w[3, :32] *= 2.0 ** 120            # and towards 252
    return w


def test_quantiser_blocks_scales_and_error():
    w = _weight(8, 128, 0)
    codes, scale = ref.quantize_weight_mxfp4(w)
    assert codes.shape == (8, 64) and scale.shape == (8, 4)
    assert codes.dtype == scale.dtype == U8
    assert 2 <= int(scale.min()) and int(scale.max()) <= 252
    p2 = torch.ldexp(torch.ones(8, 4), scale.int() - 127)
    amax = w.reshape(8, 4, 32).abs().amax(-1)
    free = (scale > 2) & (scale < 252) & (amax > 0)
    assert bool((amax / p2 <= 6).all())
    assert bool((amax / p2 > 3)[free].all())
    deq = ref.dequantize_weight_mxfp4(codes, scale)
    bound = 0.25 * torch.maximum(w.abs(), p2.repeat_interleave(32, 1))
    assert bool(((deq - w).abs() <= bound).all())
    assert int(scale[1, 1]) == 127 and not bool(codes[1, 16:32].any())


def test_ties_go_to_the_even_code_and_packing_order():
    # amax 6 -> p = 0; the midpoints of the grid, then filler
    row = torch.zeros(32)
    row[:8] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    row[8:12] = torch.tensor([-0.75, -5.0, 0.5, -1.5])
    codes, scale = ref.quantize_weight_mxfp4(row[None])
    assert int(scale) == 127
    nib = [7, 0, 2, 2, 4, 4, 6, 6, 8 | 2, 8 | 6, 1, 8 | 3]
    want = [nib[i] | (nib[i + 1] << 4) for i in range(0, 12, 2)]
    assert codes[0, :6].tolist() == want and not bool(codes[0, 6:].any())
    deq = ref.dequantize_weight_mxfp4(codes, scale)[0]
    assert deq[:12].tolist() == [6, 0, 1, 1, 2, 2, 4, 4, -1, -4, 0.5, -1.5]


@pytest.mark.parametrize("ep", [(False, None, False), (True, "gelu", True)])
def test_twin_and_cpu_fallback(ep):
    bias, act, res = ep
    g = torch.Generator().manual_seed(4)
    x = torch.randn(6, 160, generator=g)
    codes, scale = ref.quantize_weight_mxfp4(_weight(24, 160, 5))
    codes, scale = codes[:, :], scale.clamp(100, 140)  # keep fp32 finite
    b = torch.randn(24, generator=g) if bias else None
    r = torch.randn(6, 24, generator=g) if res else None
    got = ref.decode_linear_mxfp4(x, codes, scale, b, r, act)
    D = ref.dequantize_weight_mxfp4(codes, scale).to(F64)
    want = x.to(F64) @ D.t()
    mag = x.to(F64).abs() @ D.abs().t()
    if not bias:  # fp32 accumulation of K exact-in-float64 products
        assert bool(((got.to(F64) - want).abs()
                     <= 160 * 2.0 ** -23 * mag + 2.0 ** -126).all())
    # K % 128 != 0, fp32 x, leading dimensions: the op is the twin
    op = decode_linear(x.view(2, 3, 160), codes, b,
                       r.view(2, 3, 24) if res else None, act,
                       weight_scale=scale)
    assert op.shape == (2, 3, 24) and torch.equal(op.view(6, 24), got)


def test_op_errors_name_weight_scale():
    x = torch.randn(4, 128)
    codes, scale = ref.quantize_weight_mxfp4(torch.randn(16, 128))
    with pytest.raises(ValueError, match="weight_scale"):
        decode_linear(x, codes)
    with pytest.raises(ValueError, match="weight_scale"):
        decode_linear(x, codes, weight_scale=torch.ones(16))
    with pytest.raises(ValueError, match="weight_scale"):
        decode_linear(x, torch.randn(16, 128), weight_scale=scale)


def test_generation_flag_and_weight_codes():
    torch.manual_seed(11)
    gpt = GPTModel(vocab_size=512, hidden_size=128, num_layers=2,
                   num_attention_heads=2, max_position_embeddings=64,
                   hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                   fused_attn=False).eval()
    cfg = {"static_kv_cache": True, "max_dec_len": 2}
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        GPTForGeneration(gpt, dict(cfg, decode_weight_dtype="mxfp4"))
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        GPTForGeneration(gpt, dict(cfg, fused_decode_linear=True,
                                   decode_weight_dtype="mxfp8"))
    gen = GPTForGeneration(gpt, dict(cfg, fused_decode_linear=True,
                                     decode_weight_dtype="mxfp4"))
    assert gen.decode_weight_dtype == "mxfp4"
    assert gen._weight_codes.format == "mxfp4"
    assert DecodeWeightCodes().format == "fp8"
    assert list(gen.state_dict()) == list(GPTForGeneration(gpt, {}).state_dict())

    store = DecodeWeightCodes("mxfp4")
    w = torch.nn.Parameter(torch.randn(24, 160))  # K % 128 != 0 is fine
    c, s = store.get(w)
    assert c.shape == (24, 80) and s.shape == (24, 5)
    assert c.dtype == s.dtype == U8 and store.nbytes == 24 * 80 + 24 * 5
    cq, sq = ref.quantize_weight_mxfp4(w.detach())
    assert torch.equal(c, cq) and torch.equal(s, sq)
    with torch.no_grad():
        w.mul_(3.0)
    c2, s2 = store.get(w)
    assert c2 is c and s2 is s and len(store) == 1  # refreshed in place
    cq, sq = ref.quantize_weight_mxfp4(w.detach())
    assert torch.equal(c, cq) and torch.equal(s, sq)
