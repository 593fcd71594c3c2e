"""GPU: the wide MXFP4 decode_linear kernel
(csrc/decode_linear_wide_mxfp4.hip, 17 to 64 rows, x through an LDS slab)
against float64: exact decode through the slab, every instance, masking,
isolation, determinism, refusals, and batch 17 on the tiny GPT.

Accuracy bound: the MXFP4 sibling's, unchanged (derivation in
test_decode_linear_mxfp4_gpu.py), D the dequantised matrix,
r = act(x D^T + b) + res in float64, S = |x| |D|^T + |b| + |res|:

    |y - r| <= 2^-8 |r| + 2 K 2^-24 S + 2^-126

plus FP32_TOL["bg.y"] with gelu.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_decode_linear_mxfp4_gpu import (EPILOGUES, NEW, _assert_same, _cfg,
                                          _generate, _prompt,
                                          gpt)  # noqa: F401 (gpt: a fixture)
from test_decode_linear_gpu import _gelu64
from test_ops_edges_gpu import FP32_TOL

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_linear, hip_ext
from paddlefleetx_amd.parallel.env import init_dist_env

DEV = "cuda:0"
BF16, F64, F32, U8 = torch.bfloat16, torch.float64, torch.float32, torch.uint8

# (24, 512): one and a half row tiles, 4 k-steps (all tail, fewer than the
# rings hold). (136, 640): several workgroups or a partial one, 5 k-steps.
# (2048, 4224): 33 k-steps, the unrolled steady state plus a tail.
# (50304, 512): a vocabulary-sized grid.
MS = [17, 32, 33, 48, 49, 64]
CASES = [(n, k, m) for (n, k) in [(24, 512), (136, 640), (2048, 4224)]
         for m in MS] + [(50304, 512, 17), (50304, 512, 64)]
# rows per wave x waves x nontemporal: every kernel instance of each MT
VARIANTS = [(rows, waves, nt) for rows in (8, 16, 32, 64)
            for waves in (4, 8) for nt in (0, 1)]
_INPUTS, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


def _inputs(N, K):
    """64 rows of x, codes, scales, bias and residual for one (N, K); smaller
    M are leading-row slices."""
    if (N, K) not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * N + K)
        x = torch.randn(64, K, generator=g).to(BF16).to(DEV)
        w = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
        b = torch.randn(N, generator=g).to(BF16).to(DEV)
        r = torch.randn(64, N, generator=g).to(BF16).to(DEV)
        _INPUTS[(N, K)] = (x, *ref.quantize_weight_mxfp4(w), b, r)
    return _INPUTS[(N, K)]


def _reference(N, K, ep):
    """float64 (r, S) for all 64 rows, computed once and never modified."""
    if (N, K, ep) not in _REFS:
        x, c, sc, b, r = _inputs(N, K)
        bias, act, res = EPILOGUES[ep]
        D = ref.dequantize_weight_mxfp4(c, sc).to(F64)
        y, s = x.to(F64) @ D.t(), x.to(F64).abs() @ D.abs().t()
        if bias:
            y, s = y + b.to(F64), s + b.to(F64).abs()
        if act == "gelu":
            y = _gelu64(y)
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
    print(f"\n[decode_linear_wide_mxfp4] {N}x{K} M={M} {ep} {what}: worst "
          f"err/bound = {ratio:.3g}", end="")
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


@pytest.mark.parametrize("j", range(8))
def test_decode_is_exact_through_the_slab(j):
    """x row m is one-hot at k = 8 m + j: the eight cases read every k of the
    four slabs back once, through every slab row, 16-byte piece and lane
    group. Pins the slab layout and padding, the fragment addressing, the
    nibble order and the k permutation."""
    g = torch.Generator().manual_seed(7)
    codes = torch.randint(0, 256, (16, 256), generator=g, dtype=U8)
    e = torch.tensor([2, 252, 127, 119, 140], dtype=U8)
    scale = e[(torch.arange(16)[:, None] + torch.arange(16)[None]) % 5]
    ks = 8 * torch.arange(64) + j
    x = torch.zeros(64, 512, dtype=BF16)
    x[torch.arange(64), ks] = 1.0
    y = hip_ext().decode_linear_wide_mxfp4(x.to(DEV), codes.to(DEV),
                                           scale.to(DEV))
    want = ref.dequantize_weight_mxfp4(codes, scale)[:, ks].t()
    assert torch.equal(y.float().cpu(), want)


@pytest.mark.parametrize("ep", ["none", "bias_gelu", "bias_res"])
@pytest.mark.parametrize("N,K,M", CASES)
def test_accuracy_against_float64(N, K, M, ep):
    args = _args(N, K, M, ep)
    direct = hip_ext().decode_linear_wide_mxfp4(*args)
    _check(direct, N, K, M, ep, "auto")
    # the op takes the kernel: same bits as the binding called directly
    assert torch.equal(_op(*args), direct)


@pytest.mark.parametrize("N,K,M", [(136, 640, 17), (136, 640, 33),
                                   (136, 640, 64), (2048, 4224, 64)])
def test_every_kernel_instance_is_accurate(N, K, M):
    args = _args(N, K, M, "bias_res")
    for v in VARIANTS:
        got = hip_ext().decode_linear_wide_mxfp4(*args, *v)
        _check(got, N, K, M, "bias_res", f"rows/waves/nt={v}")


@pytest.mark.parametrize("M", [17, 49])
def test_nothing_past_the_ends_is_read(M):
    """Code and scale rows past N hold 0xFF (a NaN scale), x rows past M are
    NaN: none of it reaches the result, in any instance (the largest
    workgroup, 8 waves of 64 rows, reaches row N + 511)."""
    N, K = 136, 640
    x, c, sc, b, r, act = _args(N, K, M, "bias_gelu")
    xbuf = torch.full((80, K), float("nan"), dtype=BF16, device=DEV)
    cbuf = torch.full((N + 520, K // 2), 0xFF, dtype=U8, device=DEV)
    sbuf = torch.full((N + 520, K // 32), 0xFF, dtype=U8, device=DEV)
    xbuf[:M], cbuf[:N], sbuf[:N] = x, c, sc
    for v in [()] + VARIANTS:
        got = hip_ext().decode_linear_wide_mxfp4(xbuf[:M], cbuf[:N], sbuf[:N],
                                                 b, r, act, *v)
        clean = hip_ext().decode_linear_wide_mxfp4(x, c, sc, b, r, act, *v)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, clean), v


@pytest.mark.parametrize("N,K", [(24, 512), (136, 640)])
@pytest.mark.parametrize("M", [17, 33])
def test_rows_are_isolated(N, K, M):
    """An inf in the first row, then in the last (alone in its column tile):
    every other row keeps its bits."""
    x, *rest = _args(N, K, M, "bias_res")
    clean = _op(x, *rest)
    for hit in (0, M - 1):
        bad = x.clone()
        bad[hit, K // 2 + 3] = float("inf")
        got = _op(bad, *rest)
        keep = torch.arange(M, device=DEV) != hit
        assert torch.equal(got[keep], clean[keep])
        assert not bool(torch.isfinite(got[hit]).any())


@pytest.mark.parametrize("N,K,M", [(24, 512, 17), (2048, 4224, 49),
                                   (50304, 512, 64)])
def test_two_calls_are_bitwise_equal(N, K, M):
    args = _args(N, K, M, "bias_gelu")
    assert torch.equal(_op(*args), _op(*args))


def test_binding_refuses_and_op_falls_back():
    g = torch.Generator().manual_seed(3)
    ext = hip_ext()

    def rnd(*shape, dtype=BF16):
        return (torch.randn(*shape, generator=g) * 0.1).to(dtype).to(DEV)

    def q(N, K):
        return ref.quantize_weight_mxfp4(rnd(N, K, dtype=F32))

    c, s = q(24, 512)
    c384, s384 = q(24, 384)
    c576, s576 = q(24, 576)
    c20, s20 = q(20, 512)
    c1k, s1k = q(24, 1024)
    c25, s25 = q(25, 512)
    odd = c25.flatten()[8:8 + 24 * 256].view(24, 256)  # misaligned codes
    torch.cuda.synchronize()
    for bad in (dict(x=rnd(16, 512)), dict(x=rnd(65, 512)),          # M
                dict(x=rnd(20, 384), wq=c384, w_scale=s384),         # K < 512
                dict(x=rnd(20, 576), wq=c576, w_scale=s576),         # K % 128
                dict(wq=c20, w_scale=s20),                           # N = 20
                dict(wq=c1k[:, ::2]), dict(wq=odd),
                dict(wq=c.view(torch.int8)),
                dict(w_scale=s[:, :8].contiguous()), dict(w_scale=s.float()),
                dict(w_scale=s.cpu()), dict(w_scale=s.t().contiguous().t()),
                dict(x=rnd(20, 512, dtype=F32)),
                dict(rows=4), dict(rows=128), dict(waves=2), dict(waves=16),
                dict(nontemporal=2), dict(act="relu"),
                dict(bias=rnd(16)), dict(residual=rnd(16, 24))):
        kw = dict(x=rnd(20, 512), wq=c, w_scale=s)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="decode_linear_wide_mxfp4"):
            ext.decode_linear_wide_mxfp4(**kw)
    torch.cuda.synchronize()  # nothing was left in flight to fail later
    x65 = rnd(65, 512)  # M = 65: the op still computes the twin
    assert torch.equal(decode_linear(x65, c, weight_scale=s),
                       ref.decode_linear_mxfp4(x65, c, s))


def test_captured_equals_eager_at_batch_17(gpt, monkeypatch):  # noqa: F811
    calls = {}
    ext = hip_ext()
    from paddlefleetx_amd.ops import functional
    real = functional.hip_ext

    class Counting:
        def __getattr__(self, name):
            calls[name] = calls.get(name, 0) + 1
            return getattr(ext, name)

    monkeypatch.setattr(functional, "hip_ext", lambda: Counting())
    cfg = dict(_cfg("bf16"), decode_weight_dtype="mxfp4")
    eager = GPTForGeneration(gpt, cfg)
    captured = GPTForGeneration(gpt, dict(cfg, capture_decode=True))
    ids = _prompt(17, 3)
    e1 = _generate(eager, ids, 21)
    # The fixture's hidden size is 128, so only ffn_down (K = 512) meets the
    # kernel's K >= 512: one call per layer and decode step. qkv, out_proj,
    # ffn_up and the logits (K = 128) stay on the twin; the M <= 16 kernel is
    # never called at this batch.
    assert calls.get("decode_linear_wide_mxfp4", 0) == \
        (NEW - 1) * len(gpt.layers)
    assert calls.get("decode_linear_mxfp4", 0) == 0
    monkeypatch.setattr(functional, "hip_ext", real)
    _assert_same(_generate(captured, ids, 21), e1)
    ids2 = _prompt(17, 4)  # a second prompt replays the same graph
    _assert_same(_generate(captured, ids2, 22), _generate(eager, ids2, 22))
