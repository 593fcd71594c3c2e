"""GPU: the MXFP4-weight decode_linear kernel (csrc/decode_linear_mxfp4.hip):
exact decode, accuracy against float64, every variant, masking, isolation,
determinism, refusals, and the mxfp4 decode weights on a tiny GPT.

Accuracy bound (derived, not tuned), D the dequantised matrix,
r = act(x D^T + b) + res in float64, S = |x| |D|^T + |b| + |res|:

    |y - r| <= 2^-8 |r| + 2 K 2^-24 S + 2^-126

The codes decode exactly to bf16, so this is the bf16 kernel's bound (fp32
accumulation of K exact products, one rounding to bf16); with gelu the
project's fp32 bias-gelu tolerance is added.
"""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_decode_linear_fp8_gpu import (EPILOGUES, NEW, VARIANTS,
                                        _assert_same, _cfg, _generate,
                                        _linear_weights, _one_step, _prompt,
                                        gpt)  # noqa: F401 (gpt: a fixture)
from test_ops_edges_gpu import FP32_TOL

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_linear, hip_ext
from paddlefleetx_amd.parallel.env import init_dist_env

DEV = "cuda:0"
BF16, F64, F32, U8 = torch.bfloat16, torch.float64, torch.float32, torch.uint8

# one step; partial tile, 3 steps (waves with none); 33 steps in uneven
# chunks, N % 16 != 0; many tiles, short K; a vocabulary-sized grid
SHAPES = [(16, 128), (24, 384), (136, 4224), (512, 128), (50304, 128)]
CASES = [(n, k, m) for (n, k) in SHAPES for m in (1, 2, 5, 16)] \
    + [(2048, 8192, 16)]
_INPUTS, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


def _inputs(N, K):
    """16 rows of x, codes, scales, bias, residual for one (N, K), shared by
    every case of the shape (smaller M are leading-row slices)."""
    if (N, K) not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * N + K)
        x = torch.randn(16, K, generator=g).to(BF16).to(DEV)
        w = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
        b = torch.randn(N, generator=g).to(BF16).to(DEV)
        r = torch.randn(16, N, generator=g).to(BF16).to(DEV)
        _INPUTS[(N, K)] = (x, *ref.quantize_weight_mxfp4(w), b, r)
    return _INPUTS[(N, K)]


def _reference(N, K, ep):
    """float64 (r, S) for all 16 rows, computed once and never modified."""
    if (N, K, ep) not in _REFS:
        x, c, sc, b, r = _inputs(N, K)
        bias, act, res = EPILOGUES[ep]
        D = ref.dequantize_weight_mxfp4(c, sc).to(F64)
        y, s = x.to(F64) @ D.t(), x.to(F64).abs() @ D.abs().t()
        if bias:
            y, s = y + b.to(F64), s + b.to(F64).abs()
        if act == "gelu":
            y = 0.5 * y * (1.0 + torch.tanh(
                0.7978845608028654 * (y + 0.044715 * y ** 3)))
        if res:
            y, s = y + r.to(F64), s + r.to(F64).abs()
        _REFS[(N, K, ep)] = (y, s)
    return _REFS[(N, K, ep)]


def _check(got, N, K, M, ep, what):
    want, s = (t[:M] for t in _reference(N, K, ep))
    assert got.dtype == BF16 and got.shape == want.shape, what
    bound = 2.0 ** -8 * want.abs() + 2 * K * 2.0 ** -24 * s + 2.0 ** -126
    if EPILOGUES[ep][1] == "gelu":
        rtol, atol = FP32_TOL["bg.y"]
        bound = bound + atol + rtol * want.abs()
    err = (got.to(F64) - want).abs()
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max())
    print(f"\n[decode_linear_mxfp4] {what}: worst err/bound = {ratio:.3g}",
          end="")
    assert ratio <= 1.0, f"{what}: {ratio:.3g} x bound"


def _args(N, K, M, ep):
    """(x, codes, scale, bias, residual, act) as the binding takes them"""
    x, c, s, b, r = _inputs(N, K)
    bias, act, res = EPILOGUES[ep]
    return (x[:M], c, s, b if bias else None, r[:M] if res else None,
            act or "none")


def _op(x, c, s, b, r, act):
    return decode_linear(x, c, b, r, None if act == "none" else act,
                         weight_scale=s)


@pytest.mark.parametrize("j", range(16))
def test_decode_is_exact(j):
    """x row m is one-hot at k = 16 m + j: over the 16 cases every k of both
    steps, so every (lane group, word, byte, nibble), is read back. This pins
    the nibble order, the k permutation and the hardware's code table."""
    g = torch.Generator().manual_seed(7)
    codes = torch.randint(0, 256, (16, 128), generator=g, dtype=U8)
    nib = torch.cat((codes & 15, codes >> 4), 1)
    assert all(len(set(row.tolist())) == 16 for row in nib)
    e = torch.tensor([2, 252, 127, 119, 140], dtype=U8)
    scale = e[(torch.arange(16)[:, None] + torch.arange(8)[None]) % 5]
    ks = 16 * torch.arange(16) + j
    x = torch.zeros(16, 256, dtype=BF16)
    x[torch.arange(16), ks] = 1.0
    y = hip_ext().decode_linear_mxfp4(x.to(DEV), codes.to(DEV), scale.to(DEV))
    want = ref.dequantize_weight_mxfp4(codes, scale)[:, ks].t()
    assert torch.equal(y.float().cpu(), want)


@pytest.mark.parametrize("ep", list(EPILOGUES))
@pytest.mark.parametrize("N,K,M", CASES)
def test_accuracy_against_float64(N, K, M, ep):
    args = _args(N, K, M, ep)
    got = _op(*args)
    _check(got, N, K, M, ep, f"{N}x{K} M={M} {ep}")
    # the op took the kernel: same bits as the binding called directly
    assert torch.equal(got, hip_ext().decode_linear_mxfp4(*args))


@pytest.mark.parametrize("rows,waves,nt", VARIANTS)
@pytest.mark.parametrize("N,K,M", [(24, 384, 5), (136, 4224, 16)])
def test_every_kernel_variant_is_accurate(N, K, M, rows, waves, nt):
    got = hip_ext().decode_linear_mxfp4(*_args(N, K, M, "bias_res"), rows,
                                        waves, nt)
    _check(got, N, K, M, "bias_res",
           f"{N}x{K} M={M} rows={rows} waves={waves} nt={nt}")


@pytest.mark.parametrize("M", [1, 5, 16])
def test_rows_past_m_and_n_are_never_read(M):
    """Code and scale rows past N hold 0xFF (a NaN scale), x rows past M are
    NaN: none of it reaches the result, in any variant (64-row workgroups
    reach row N + 63)."""
    N, K = 24, 384
    x, c, sc, b, r = _inputs(N, K)
    xbuf = torch.full((32, K), float("nan"), dtype=BF16, device=DEV)
    cbuf = torch.full((N + 72, K // 2), 0xFF, dtype=U8, device=DEV)
    sbuf = torch.full((N + 72, K // 32), 0xFF, dtype=U8, device=DEV)
    xbuf[:M], cbuf[:N], sbuf[:N] = x[:M], c, sc
    for v in [()] + VARIANTS:
        got = hip_ext().decode_linear_mxfp4(xbuf[:M], cbuf[:N], sbuf[:N], b,
                                            r[:M], "gelu", *v)
        clean = hip_ext().decode_linear_mxfp4(x[:M], c, sc, b, r[:M], "gelu",
                                              *v)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, clean), v


@pytest.mark.parametrize("N,K,M", [(24, 384, 5), (136, 4224, 16)])
def test_rows_are_isolated_and_calls_deterministic(N, K, M):
    args = _args(N, K, M, "bias_res")
    clean = _op(*args)
    assert torch.equal(clean, _op(*args))
    bad = args[0].clone()
    bad[0, K // 2 + 3] = float("inf")
    got = _op(bad, *args[1:])
    assert torch.equal(got[1:], clean[1:])
    assert not bool(torch.isfinite(got[0]).any())


def test_binding_refuses_and_op_falls_back():
    g = torch.Generator().manual_seed(3)
    ext = hip_ext()

    def rnd(*shape, dtype=BF16):
        return (torch.randn(*shape, generator=g) * 0.1).to(dtype).to(DEV)

    def q(N, K):
        return ref.quantize_weight_mxfp4(rnd(N, K, dtype=F32))

    c, s = q(24, 256)
    c25, s25 = q(25, 128)
    odd = c25.flatten()[8:8 + 24 * 64].view(24, 64)  # misaligned codes
    for x, cc, ss in [(rnd(17, 128), *q(24, 128)),             # M = 17
                      (rnd(4, 64), *q(24, 64)),                # K = 64
                      (rnd(4, 192), *q(24, 192)),              # K = 192
                      (rnd(4, 128), *q(20, 128)),              # N = 20
                      (rnd(4, 128, dtype=F32), *q(24, 128)),   # fp32 x
                      (rnd(4, 128), c[:, ::2], s[:, :4].contiguous()),
                      (rnd(4, 128), odd, s25[:24].contiguous())]:
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="decode_linear_mxfp4"):
            ext.decode_linear_mxfp4(x, cc, ss)
        torch.cuda.synchronize()  # nothing was left in flight to fail later
        assert torch.equal(decode_linear(x, cc, weight_scale=ss),
                           ref.decode_linear_mxfp4(x, cc, ss))
    c, s = q(24, 128)
    for bad in (dict(w_scale=s[:, :2].contiguous()), dict(w_scale=s.float()),
                dict(w_scale=s.cpu()), dict(w_scale=s.t().contiguous().t()),
                dict(wq=c.view(torch.int8)), dict(rows=4), dict(rows=128),
                dict(waves=2), dict(nontemporal=2), dict(act="relu")):
        kw = dict(x=rnd(4, 128), wq=c, w_scale=s)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="decode_linear_mxfp4"):
            ext.decode_linear_mxfp4(**kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_captured_equals_eager_with_mxfp4_weights(gpt, kv, monkeypatch):
    calls = {"decode_linear_mxfp4": 0, "decode_linear_fp8": 0,
             "decode_linear": 0}
    ext = hip_ext()
    from paddlefleetx_amd.ops import functional
    real = functional.hip_ext

    class Counting:
        def __getattr__(self, name):
            calls[name] = calls.get(name, 0) + 1
            return getattr(ext, name)

    monkeypatch.setattr(functional, "hip_ext", lambda: Counting())
    cfg = dict(_cfg(kv), decode_weight_dtype="mxfp4")
    eager = GPTForGeneration(gpt, cfg)
    captured = GPTForGeneration(gpt, dict(cfg, capture_decode=True))
    ids = _prompt(2, 3)
    e1 = _generate(eager, ids, 21)
    # the kernel itself ran: 4 per layer + the logits, every decode step
    assert calls["decode_linear_mxfp4"] == \
        (NEW - 1) * (4 * len(gpt.layers) + 1)
    assert calls["decode_linear"] == calls["decode_linear_fp8"] == 0
    monkeypatch.setattr(functional, "hip_ext", real)
    _assert_same(_generate(captured, ids, 21), e1)
    ids2 = _prompt(2, 4)  # a second prompt replays the same graph
    _assert_same(_generate(captured, ids2, 22), _generate(eager, ids2, 22))


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_teacher_forced_step_is_no_worse_than_existing_path(gpt, kv):
    """The rule of the fp8 test: reference, the fp32 model holding the
    dequantised weights; off, the bf16 fused path on those weights; on, the
    mxfp4 path of the unchanged model."""
    cfg = dict(static_kv_cache=True, kv_cache_dtype=kv, max_dec_len=2,
               fused_decode_linear=True)
    gen_off = GPTForGeneration(gpt, cfg)
    gen_on = GPTForGeneration(gpt, dict(cfg, decode_weight_dtype="mxfp4"))
    gpt32 = copy.deepcopy(gpt).float()
    deq32, deq16 = copy.deepcopy(gpt32), copy.deepcopy(gpt)
    with torch.no_grad():
        for w, w32, w16 in zip(_linear_weights(gpt), _linear_weights(deq32),
                               _linear_weights(deq16)):
            d = ref.dequantize_weight_mxfp4(*ref.quantize_weight_mxfp4(w))
            w32.copy_(d)
            w16.copy_(d)  # exact: every decoded value is a bf16
    for m in (gpt32, deq32):
        for layer in m.layers:
            layer.attn.fused_attn = False  # the flash kernel is bf16 only
    ids, tok = _prompt(4, 7), _prompt(4, 8)[:, :1].contiguous()
    plain = GPTForGeneration(gpt, dict(static_kv_cache=True,
                                       kv_cache_dtype=kv, max_dec_len=2))
    want = _one_step(plain, deq32, ids, tok, prefill_model=gpt32)
    e_off = float((_one_step(gen_off, deq16, ids, tok, prefill_model=gpt)
                   - want).abs().max())
    h_on = _one_step(gen_on, gpt, ids, tok)
    e_on = float((h_on - want).abs().max())
    d_q = float((h_on - _one_step(gen_off, gpt, ids, tok)).abs().max())
    print(f"\n[decode_linear_mxfp4] step {kv}: error vs fp32 dequantised "
          f"reference: mxfp4 {e_on:.3e}, bf16 path {e_off:.3e}; distance "
          f"from the unquantised step {d_q:.3e} (information)", end="")
    assert e_off > 0 and torch.isfinite(h_on).all()
    assert e_on <= 2 * e_off, (e_on, e_off)
