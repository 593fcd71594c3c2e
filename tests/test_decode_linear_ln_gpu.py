"""GPU: the LayerNorm-prologue decode_linear kernels (bf16 and fp8 weights)
against float64, their second variance pass, isolation, refusals, and
Generation.fused_decode_ln on the tiny GPT of test_decode_linear_gpu.py.

Bound (derived; extends test_decode_linear_gpu.py). In float64 from the same
bf16 inputs: n = (x - mu) / sqrt(var + eps), h = n g + b, Ht = |n||g| + |b|,
r = act(h W^T (* scale) + bias) + res, S = Ht |W|^T (* scale) + |bias| + |res|:

    |y - r| <= 2^-8 |r| + (2^-8 + c K 2^-24) S + 2^-126

c = 2 (bf16 weights) or (2K + 2) / K (fp8: the scale multiply). 2^-8 S is
the one new rounding: h to bf16 (half an ulp, 2^-9) and as much again for
the fp32 evaluation of the statistics and of h. GELU adds FP32_TOL["bg.y"].
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_decode_linear_gpu import (_assert_same, _cfg, _env,  # noqa
                                    _generate, _one_step, _prompt, gpt)
from test_ops_edges_gpu import FP32_TOL

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_linear, hip_ext, layernorm

DEV, BF16, F64, EPS = "cuda:0", torch.bfloat16, torch.float64, 1e-5
WDS = ["bf16", "fp8"]
SHAPES = {"bf16": [(16, 64), (24, 96), (128, 512), (2048, 2080)],
          "fp8": [(16, 64), (128, 512), (2048, 2112)]}
# (bias, activation, residual)
EPILOGUES = {"none": (False, None, False), "bias_gelu": (True, "gelu", False),
             "bias_res": (True, None, True)}
_CACHE = {}


def _rows(K, g, far=False):
    """16 rows randn * sigma_m + mu_m, sigma over [0.5, 4], |mu| <= 4 sigma
    (far: 1000 sigma), alternating sign: statistics of a wrong row show."""
    sigma = torch.linspace(0.5, 4.0, 16)[:, None]
    m = torch.arange(16)[:, None]
    mu = sigma * (1000.0 if far else (m % 5).float()) * (1 - 2 * (m % 2))
    return (torch.randn(16, K, generator=g) * sigma + mu).to(BF16).to(DEV)


def _pack(w, wd, exact=False):
    """(weight or codes, scale or None, float64 weight without the scale)"""
    if wd == "bf16":
        return w, None, w.to(F64)
    if exact:  # the code of 1.0 with scale 1
        c, s = w.to(torch.float8_e4m3fn), torch.ones(w.shape[0], device=DEV)
    else:
        c, s = ref.quantize_weight_rows(w)
    return c, s, c.float().to(F64)


def _inputs(N, K, wd):
    key = (N, K, wd)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * N + K)
        x = _rows(K, g)
        w = (torch.randn(N, K, generator=g) * 0.05).to(BF16).to(DEV)
        b, r = (torch.randn(*s, generator=g).to(BF16).to(DEV)
                for s in ((N,), (16, N)))
        ln = tuple(torch.randn(K, generator=g).to(BF16).to(DEV)
                   for _ in range(2)) + (EPS,)
        _CACHE[key] = (x, _pack(w, wd), b, r, ln)
    return _CACHE[key]


def _reference(x, pack, b, r, ln, act):
    """float64 (r, S) of the docstring; b / r None when absent"""
    x64, (lw, lb, eps), (_, scale, w64) = x.to(F64), ln, pack
    mu = x64.mean(-1, keepdim=True)
    n = (x64 - mu) / (x64.var(-1, unbiased=False, keepdim=True) + eps).sqrt()
    y = (n * lw.to(F64) + lb.to(F64)) @ w64.t()
    s = (n.abs() * lw.to(F64).abs() + lb.to(F64).abs()) @ w64.abs().t()
    if scale is not None:
        y, s = y * scale.to(F64), s * scale.to(F64)
    if b is not None:
        y, s = y + b.to(F64), s + b.to(F64).abs()
    if act == "gelu":
        y = torch.nn.functional.gelu(y, approximate="tanh")
    if r is not None:
        y, s = y + r.to(F64), s + r.to(F64).abs()
    return y, s


def _check(got, want, s, K, wd, gelu, what):
    assert got.dtype == BF16 and got.shape == want.shape, what
    ck = 2 * K if wd == "bf16" else 2 * K + 2
    bound = 2.0 ** -8 * want.abs() + (2.0 ** -8 + ck * 2.0 ** -24) * s \
        + 2.0 ** -126
    if gelu:
        rtol, atol = FP32_TOL["bg.y"]
        bound = bound + atol + rtol * want.abs()
    err = (got.to(F64) - want).abs()
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max())
    print(f"\n[decode_linear_ln] {what}: worst err/bound = {ratio:.3g}",
          end="")
    assert ratio <= 1.0, f"{what}: {ratio:.3g} x bound"


def _direct(x, pack, b, r, act, ln, *variant):
    """the binding itself; variant = (rows, waves, nontemporal)"""
    kw = dict(ln_weight=ln[0], ln_bias=ln[1], ln_eps=ln[2])
    args = (b, r, act or "none") + variant
    if pack[1] is None:
        return hip_ext().decode_linear(x, pack[0], *args, **kw)
    return hip_ext().decode_linear_fp8(x, pack[0], pack[1], *args, **kw)


def _op(x, pack, b=None, r=None, act=None, ln=None):
    return decode_linear(x, pack[0], b, r, act, weight_scale=pack[1], ln=ln)


def _case(N, K, M, wd, ep):
    x, pack, b, r, ln = _inputs(N, K, wd)
    bias, act, res = EPILOGUES[ep]
    return x[:M], pack, b if bias else None, r[:M] if res else None, act, ln


@pytest.mark.parametrize("ep", list(EPILOGUES))
@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("wd,N,K", [(wd, n, k) for wd in WDS
                                    for n, k in SHAPES[wd]])
def test_accuracy_against_float64(wd, N, K, M, ep):
    x, pack, b, r, act, ln = _case(N, K, M, wd, ep)
    got = _op(x, pack, b, r, act, ln)
    want, s = _reference(x, pack, b, r, ln, act)
    _check(got, want, s, K, wd, act == "gelu", f"{wd} {N}x{K} M={M} {ep}")
    # the op took the kernel: same bits as the binding called directly
    assert torch.equal(got, _direct(x, pack, b, r, act, ln))


@pytest.mark.parametrize("wd,N,K,M,rows,waves,nt", [
    (wd, n, k, m, rows, waves, nt)
    for wd, n, k, m in [("bf16", 24, 96, 5), ("bf16", 2048, 2080, 16),
                        # fp8 needs K % 64 == 0
                        ("fp8", 24, 128, 5), ("fp8", 2048, 2112, 16)]
    for rows in (8, 16, 32) + ((64,) if wd == "fp8" else ())
    for waves in (4, 8) for nt in (0, 1)])
def test_every_kernel_variant_is_accurate(wd, N, K, M, rows, waves, nt):
    x, pack, b, r, act, ln = _case(N, K, M, wd, "bias_res")
    got = _direct(x, pack, b, r, act, ln, rows, waves, nt)
    want, s = _reference(x, pack, b, r, ln, act)
    _check(got, want, s, K, wd, False,
           f"{wd} {N}x{K} M={M} rows={rows} waves={waves} nt={nt}")


@pytest.mark.parametrize("K", [128, 512])
@pytest.mark.parametrize("wd", WDS)
def test_second_variance_pass(wd, K):
    """Identity weight: y = bf16(h), so the bound is sharp on the
    statistics. With |mu| = 1000 sigma a one-pass variance alone reaches 2.3
    (K = 128) and 7.4 (K = 512) times the bound, two passes stay at 0.49."""
    g = torch.Generator().manual_seed(K)
    x = _rows(K, g, far=True)
    ln = tuple(torch.randn(K, generator=g).to(BF16).to(DEV)
               for _ in range(2)) + (EPS,)
    pack = _pack(torch.eye(K, dtype=BF16, device=DEV), wd, exact=True)
    want, s = _reference(x, pack, None, None, ln, None)
    _check(_op(x, pack, ln=ln), want, s, K, wd, False, f"{wd} far rows K={K}")


@pytest.mark.parametrize("wd", WDS)
def test_isolation_masking_reproducibility(wd):
    x, pack, b, r, act, ln = _case(128, 512, 5, wd, "bias_res")
    clean = _op(x, pack, b, r, act, ln)
    assert torch.equal(clean, _op(x, pack, b, r, act, ln))
    buf = torch.full((16, 512), float("nan"), dtype=BF16, device=DEV)
    buf[:5] = x
    assert torch.equal(clean, _op(buf[:5], pack, b, r, act, ln))
    bad = x.clone()
    bad[2] = float("nan")
    got = _op(bad, pack, b, r, act, ln)
    assert bool(got[2].isnan().all())
    far = x.clone()
    far[2] = _rows(512, torch.Generator().manual_seed(5), far=True)[15]
    for y in (got, _op(far, pack, b, r, act, ln)):  # row 2 forces pass two
        assert torch.equal(y[[0, 1, 3, 4]], clean[[0, 1, 3, 4]])


@pytest.mark.parametrize("wd", WDS)
def test_binding_refuses_and_op_falls_back(wd):
    x, pack, _, _, _, (lw, lb, eps) = _case(128, 512, 5, wd, "none")
    odd = torch.cat([lb[:1], lb])[1:]  # same values, 2 bytes off alignment
    # (ln, whether layernorm(x, *ln) exists as a fallback value)
    for ln, falls_back in [((lw.float(), lb, eps), True),
                           ((lw, odd, eps), True), ((lw, lb, 0.0), True),
                           ((lw[:-8], lb, eps), False),
                           ((lw, None, eps), False)]:
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="decode_linear"):
            _direct(x, pack, None, None, None, ln)
        torch.cuda.synchronize()  # nothing was left in flight to fail later
        if falls_back:
            want = layernorm(x, ln[0], ln[1].clone(), ln[2])  # aligned copy
            assert torch.equal(_op(x, pack, ln=ln), _op(want, pack))
        else:  # no LayerNorm of that kind in the library either
            with pytest.raises((RuntimeError, ValueError)):
                _op(x, pack, ln=ln)


# model level: the tiny GPT of test_decode_linear_gpu.py

@pytest.mark.parametrize("wd", WDS)
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_teacher_forced_step_is_as_close_as_separate_layernorm(gpt, kv, wd):
    """Flag on and off round in the same places and differ in the fp32
    summation order of the statistics: 1.5 x the flag-off distance from the
    fp32 model, the spread KERNELS.md records between two such paths."""
    import copy
    cfg = dict(static_kv_cache=True, kv_cache_dtype=kv, max_dec_len=2,
               fused_decode_linear=True, decode_weight_dtype=wd)
    gen_off = GPTForGeneration(gpt, cfg)
    gen_on = GPTForGeneration(gpt, dict(cfg, fused_decode_ln=True))
    gpt32 = copy.deepcopy(gpt).float()
    for layer in gpt32.layers:
        layer.attn.fused_attn = False  # the flash kernel is bf16 only
    ids = _prompt(4, 7)
    tok = _prompt(4, 8)[:, :1].contiguous()
    plain = GPTForGeneration(gpt, dict(static_kv_cache=True,
                                       kv_cache_dtype=kv, max_dec_len=2))
    want = _one_step(plain, gpt32, ids, tok)
    e_off = float((_one_step(gen_off, gpt, ids, tok) - want).abs().max())
    h_on = _one_step(gen_on, gpt, ids, tok)
    e_on = float((h_on - want).abs().max())
    print(f"\n[decode_linear_ln] step kv {kv} weights {wd}: max-abs distance "
          f"from the fp32 model, flag on {e_on:.3e}, off {e_off:.3e}", end="")
    assert e_off > 0 and torch.isfinite(h_on).all()
    assert e_on <= 1.5 * e_off, (e_on, e_off)


@pytest.mark.parametrize("wd", WDS)
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_captured_equals_eager_with_fused_ln(gpt, kv, wd, monkeypatch):
    from paddlefleetx_amd.ops import functional
    calls, ext = [], hip_ext()

    class Counting:
        def __getattr__(self, name):
            if name == "layernorm_fwd":
                calls.append(1)
            return getattr(ext, name)

    cfg = _cfg(kv, fused_decode_ln=True, decode_weight_dtype=wd)
    eager = GPTForGeneration(gpt, cfg)
    captured = GPTForGeneration(gpt, dict(cfg, capture_decode=True))
    monkeypatch.setattr(functional, "hip_ext", lambda: Counting())
    ids = _prompt(2, 3)
    e1 = _generate(eager, ids, 21)
    # no decode step ran a LayerNorm of its own: ln1 of every layer and
    # final_ln of the prefill are all (its ln2 is layernorm_fwd_residual)
    assert len(calls) == len(gpt.layers) + 1
    monkeypatch.undo()
    _assert_same(_generate(captured, ids, 21), e1)
    ids2 = _prompt(2, 4)  # a second prompt replays the same graph
    _assert_same(_generate(captured, ids2, 22), _generate(eager, ids2, 22))
