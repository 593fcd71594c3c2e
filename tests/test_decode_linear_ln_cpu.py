"""decode_linear with a LayerNorm in front (ln=) without a GPU: the twins and
the op's fallback against float64 under the bound of
test_decode_linear_ln_gpu.py, and Generation.fused_decode_ln on the CPU.

    |y - r| <= eps |r| + (eps + c K 2^-24) S + 2^-126,  S = Ht |W|^T + ...

with eps = 2^-8 for bf16 and 2^-23 for fp32 (one rounding of h, one of y),
Ht = |n||g| + |b|, c = 2 (or (2K + 2) / K with fp8 codes).
"""

import pytest
import torch

from test_decode_linear_cpu import _tiny_gpt

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_linear

F64, LN_EPS = torch.float64, 1e-5


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,K,M", [(16, 64, 16), (24, 128, 5), (128, 512, 16)])
def test_twin_and_fallback_against_float64(N, K, M, dtype, fp8):
    g = torch.Generator().manual_seed(100 * N + K + M)
    sigma, m = torch.linspace(0.5, 4.0, M)[:, None], torch.arange(M)[:, None]
    mu = sigma * (m % 5) * (1 - 2 * (m % 2))
    x = (torch.randn(M, K, generator=g) * sigma + mu).to(dtype)
    w = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    b, r = torch.randn(N, generator=g).to(dtype), \
        torch.randn(M, N, generator=g).to(dtype)
    lw, lb = (torch.randn(K, generator=g).to(dtype) for _ in range(2))
    ln = (lw, lb, LN_EPS)
    scale = None
    if fp8:
        w, scale = ref.quantize_weight_rows(w)
    x64, w64 = x.to(F64), w.float().to(F64)
    n = (x64 - x64.mean(-1, keepdim=True)) / (
        x64.var(-1, unbiased=False, keepdim=True) + LN_EPS).sqrt()
    want = (n * lw.to(F64) + lb.to(F64)) @ w64.t()
    s = (n.abs() * lw.to(F64).abs() + lb.to(F64).abs()) @ w64.abs().t()
    if fp8:
        want, s = want * scale.to(F64), s * scale.to(F64)
    want = want + b.to(F64) + r.to(F64)
    s = s + b.to(F64).abs() + r.to(F64).abs()
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -23
    c = (2 * K + 2) / K if fp8 else 2
    bound = eps * want.abs() + (eps + c * K * 2.0 ** -24) * s + 2.0 ** -126
    twin = ref.decode_linear_fp8(x, w, scale, b, r, None, ln=ln) if fp8 \
        else ref.decode_linear(x, w, b, r, None, ln=ln)
    op = decode_linear(x, w, b, r, weight_scale=scale, ln=ln)
    for name, got in (("twin", twin), ("op", op)):
        assert got.dtype == dtype and got.shape == (M, N)
        ratio = float(((got.to(F64) - want).abs() / bound).max())
        print(f"\n[decode_linear_ln] cpu {name} {N}x{K} M={M} {dtype} "
              f"fp8={fp8}: worst err/bound = {ratio:.3g}", end="")
        assert ratio <= 1.0, (name, ratio)


def test_generation_flag_on_cpu():
    gpt = _tiny_gpt()
    cfg = dict(static_kv_cache=True, fused_sampling=True, max_dec_len=4,
               min_dec_len=4, decoding_strategy="greedy_search",
               eos_token_id=511, fused_decode_linear=True)
    with pytest.raises(ValueError, match="fused_decode_ln"):
        GPTForGeneration(gpt, {"static_kv_cache": True,
                               "fused_decode_ln": True})
    off = GPTForGeneration(gpt, cfg)
    on = GPTForGeneration(gpt, dict(cfg, fused_decode_ln=True))
    assert on.fused_decode_ln and not off.fused_decode_ln
    assert on._new_static_cache(1, 4, "cpu").fused_decode_ln
    assert not off._new_static_cache(1, 4, "cpu").fused_decode_ln
    ids = torch.randint(0, 511, (2, 5),
                        generator=torch.Generator().manual_seed(9))
    out = on(ids)
    assert out.shape == (2, 4) and torch.equal(out, off(ids))
    # the hidden state before final_ln is what the logits launch normalises
    pos = torch.arange(5).unsqueeze(0).expand(2, -1)
    with torch.no_grad():
        raw = gpt(ids, pos, apply_final_ln=False)
        assert torch.equal(gpt.final_ln(raw), gpt(ids, pos))
