"""GPU: the tiled GEMM over weight codes (csrc/linear_codes.hip, M >= 65, fp8
or MXFP4 weights) against float64 from the same codes: exact decode through
LDS, every instance, masking, isolation, determinism, refusals, and batch 65
on the tiny GPT.

Accuracy bounds: the siblings', unchanged (derivations in
test_decode_linear_fp8_gpu.py and test_decode_linear_mxfp4_gpu.py), D the
dequantised codes, r = act((x D^T)(scale) + b) + res in float64 and S the same
expression over absolute values:

    fp8     |y - r| <= 2^-8 |r| + (2 K + 2) 2^-24 S + 2^-126
    mxfp4   |y - r| <= 2^-8 |r| + 2 K 2^-24 S + 2^-126

plus FP32_TOL["bg.y"] with gelu.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_decode_linear_wide_mxfp4_gpu import (EPILOGUES, FP32_TOL, NEW,
                                               _assert_same, _cfg, _gelu64,
                                               _generate, _prompt,
                                               gpt)  # noqa: F401 (a fixture)

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_linear, hip_ext
from paddlefleetx_amd.parallel.env import init_dist_env

DEV = "cuda:0"
BF16, F64, F32, U8 = torch.bfloat16, torch.float64, torch.float32, torch.uint8
FP8 = torch.float8_e4m3fn
FMTS = ["fp8", "mxfp4"]

# M: one row past the wide kernels, the M tile (128) - 1, + 0, + 1, three
# tiles with a partial last. (136, 128): two slabs, N one tile + 8.
# (136, 640): 10 slabs. (392, 2176): 34 slabs, four N tiles of 128 with a
# partial last. (136, 192), fp8: 3 slabs, K no multiple of 128.
# (50304, 256): a vocabulary-sized grid.
MS = [65, 127, 128, 129, 300]
SHAPES = [(136, 128), (136, 640), (392, 2176)]
CASES = [(f, n, k, m) for f in FMTS
         for (n, k) in SHAPES + ([(136, 192)] if f == "fp8" else [])
         for m in MS] + [(f, 50304, 256, m) for f in FMTS for m in (65, 200)]
# N per workgroup tile: every instance. N = 24, 40, 56, 72 are the 32 and 64
# wide tiles - 8 and + 8 (N % 8 == 0 leaves no +- 1).
TILES = [128, 64, 32]
EDGE_N = [24, 40, 56, 72]
_INPUTS, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


def _inputs(fmt, N, K):
    """300 rows of x, codes, scales, bias and residual for one (N, K) (200 at
    the vocabulary); smaller M are leading-row slices."""
    if (fmt, N, K) not in _INPUTS:
        rows = 200 if N > 4096 else 300
        g = torch.Generator().manual_seed(1000 * N + K)
        x = torch.randn(rows, K, generator=g).to(BF16).to(DEV)
        w = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
        b = torch.randn(N, generator=g).to(BF16).to(DEV)
        r = torch.randn(rows, N, generator=g).to(BF16).to(DEV)
        q = ref.quantize_weight_mxfp4(w) if fmt == "mxfp4" \
            else ref.quantize_weight_rows(w.to(BF16))
        _INPUTS[(fmt, N, K)] = (x, *q, b, r)
    return _INPUTS[(fmt, N, K)]


def _reference(fmt, N, K, ep):
    """float64 (r, S) for every row, computed once and never modified."""
    if (fmt, N, K, ep) not in _REFS:
        x, c, sc, b, r = _inputs(fmt, N, K)
        bias, act, res = EPILOGUES[ep]
        D = ref.dequantize_weight_mxfp4(c, sc).to(F64) if fmt == "mxfp4" \
            else c.float().to(F64)
        y, s = x.to(F64) @ D.t(), x.to(F64).abs() @ D.abs().t()
        if fmt == "fp8":
            y, s = y * sc.to(F64), s * sc.to(F64)
        if bias:
            y, s = y + b.to(F64), s + b.to(F64).abs()
        if act == "gelu":
            y = _gelu64(y)
        if res:
            y, s = y + r.to(F64), s + r.to(F64).abs()
        _REFS[(fmt, N, K, ep)] = (y, s)
    return _REFS[(fmt, N, K, ep)]


def _check(got, fmt, N, K, M, ep, what):
    want, s = (t[:M] for t in _reference(fmt, N, K, ep))
    assert got.dtype == BF16 and got.shape == want.shape, what
    c = 2 * K + (2 if fmt == "fp8" else 0)
    bound = 2.0 ** -8 * want.abs() + c * 2.0 ** -24 * s + 2.0 ** -126
    if EPILOGUES[ep][1] == "gelu":
        rtol, atol = FP32_TOL["bg.y"]
        bound = bound + atol + rtol * want.abs()
    err = (got.to(F64) - want).abs()
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max())
    print(f"\n[linear_codes] {fmt} {N}x{K} M={M} {ep} {what}: worst "
          f"err/bound = {ratio:.3g}", end="")
    assert ratio <= 1.0, f"{what}: {ratio:.3g} x bound"


def _args(fmt, N, K, M, ep):
    """(x, codes, scale, bias, residual, act) as the binding takes them"""
    x, c, s, b, r = _inputs(fmt, N, K)
    bias, act, res = EPILOGUES[ep]
    return (x[:M], c, s, b if bias else None, r[:M] if res else None,
            act or "none")


def _op(x, c, s, b, r, act):
    return decode_linear(x, c, b, r, None if act == "none" else act,
                         weight_scale=s)


@pytest.mark.parametrize("tile", [0] + TILES)
@pytest.mark.parametrize("fmt", FMTS)
def test_decode_is_exact_through_lds(fmt, tile):
    """x is the identity: y is the dequantised matrix transposed, bit for
    bit. Pins the slab layout and padding, the fragment addressing, the
    nibble order and the k order."""
    g = torch.Generator().manual_seed(7)
    K, N = 256, 136
    x = torch.eye(K, dtype=BF16, device=DEV)
    if fmt == "mxfp4":
        codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=U8)
        e = torch.tensor([2, 252, 127, 119, 140], dtype=U8)
        scale = e[(torch.arange(N)[:, None] + torch.arange(K // 32)[None]) % 5]
        want = ref.dequantize_weight_mxfp4(codes, scale).t()
    else:
        codes = torch.randint(0, 256, (N, K), generator=g, dtype=U8)
        codes[(codes & 0x7F) == 0x7F] = 0x3A  # the two NaN encodings
        scale = 2.0 ** ((torch.arange(N) % 9) - 4).float()
        want = (codes.view(FP8).float() * scale[:, None]).t()
        codes = codes.view(FP8)
    y = hip_ext().linear_codes(x, codes.to(DEV), scale.to(DEV), tile_n=tile)
    assert torch.equal(y.float().cpu(), want)


@pytest.mark.parametrize("ep", ["none", "bias_gelu", "bias_res"])
@pytest.mark.parametrize("fmt,N,K,M", CASES)
def test_accuracy_against_float64(fmt, N, K, M, ep):
    args = _args(fmt, N, K, M, ep)
    direct = hip_ext().linear_codes(*args)
    _check(direct, fmt, N, K, M, ep, "auto")
    # the op takes the kernel: same bits as the binding called directly
    assert torch.equal(_op(*args), direct)


@pytest.mark.parametrize("M", [65, 129])
@pytest.mark.parametrize("N,K", [(136, 640), (392, 2176)]
                         + [(n, 128) for n in EDGE_N])
@pytest.mark.parametrize("fmt", FMTS)
def test_every_kernel_instance_is_accurate(fmt, N, K, M):
    args = _args(fmt, N, K, M, "bias_res")
    for t in TILES:
        got = hip_ext().linear_codes(*args, t)
        _check(got, fmt, N, K, M, "bias_res", f"tile_n={t}")


@pytest.mark.parametrize("M", [65, 129])
@pytest.mark.parametrize("fmt", FMTS)
def test_nothing_past_the_ends_is_read(fmt, M):
    """Code and scale rows past N hold 0xFF (NaN codes, NaN scales), x rows
    past M are NaN: none of it reaches the result, in any instance (the
    largest tile reaches row N + 119 and row M + 127)."""
    N, K = 136, 640
    x, c, sc, b, r, act = _args(fmt, N, K, M, "bias_gelu")
    xbuf = torch.full((M + 128, K), float("nan"), dtype=BF16, device=DEV)
    cbuf = torch.full((N + 128, c.shape[1]), 0xFF, dtype=U8,
                      device=DEV).view(c.dtype)
    sbuf = torch.full(((N + 128) * sc[0].numel() * sc.element_size(),), 0xFF,
                      dtype=U8, device=DEV).view(sc.dtype) \
        .view(N + 128, *sc.shape[1:])
    xbuf[:M], cbuf[:N], sbuf[:N] = x, c, sc
    for t in [0] + TILES:
        got = hip_ext().linear_codes(xbuf[:M], cbuf[:N], sbuf[:N], b, r, act,
                                     t)
        clean = hip_ext().linear_codes(x, c, sc, b, r, act, t)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, clean), t


@pytest.mark.parametrize("M", [65, 129])
@pytest.mark.parametrize("fmt", FMTS)
def test_rows_are_isolated(fmt, M):
    """An inf in the first row, then in the last (alone in its M tile at
    129): every other row keeps its bits."""
    N, K = 136, 640
    x, *rest = _args(fmt, N, K, M, "bias_res")
    clean = _op(x, *rest)
    for hit in (0, M - 1):
        bad = x.clone()
        bad[hit, K // 2 + 3] = float("inf")
        got = _op(bad, *rest)
        keep = torch.arange(M, device=DEV) != hit
        assert torch.equal(got[keep], clean[keep])
        assert not bool(torch.isfinite(got[hit]).any())


@pytest.mark.parametrize("N,K,M", [(136, 128, 65), (392, 2176, 300),
                                   (50304, 256, 200)])
@pytest.mark.parametrize("fmt", FMTS)
def test_two_calls_are_bitwise_equal(fmt, N, K, M):
    args = _args(fmt, N, K, M, "bias_gelu")
    assert torch.equal(_op(*args), _op(*args))


def test_binding_refuses_and_op_falls_back():
    g = torch.Generator().manual_seed(3)
    ext = hip_ext()

    def rnd(*shape, dtype=BF16):
        return (torch.randn(*shape, generator=g) * 0.1).to(dtype).to(DEV)

    def q8(N, K):
        return ref.quantize_weight_rows(rnd(N, K))

    def q4(N, K):
        return ref.quantize_weight_mxfp4(rnd(N, K, dtype=F32))

    c8, s8 = q8(136, 256)
    c4, s4 = q4(136, 256)
    c8k, s8k = q8(136, 96)
    c4k, s4k = q4(136, 192)
    c8n, s8n = q8(132, 256)
    c8w, _ = q8(136, 512)
    c4w, _ = q4(137, 256)
    odd = c4w.flatten()[8:8 + 136 * 128].view(136, 128)  # misaligned codes
    torch.cuda.synchronize()
    for bad in (dict(x=rnd(64, 256)),                                # M
                dict(x=rnd(70, 96), codes=c8k, w_scale=s8k),         # K % 64
                dict(x=rnd(70, 192), codes=c4k, w_scale=s4k),        # K % 128
                dict(codes=c8n, w_scale=s8n),                        # N % 8
                dict(codes=c8w[:, ::2]), dict(codes=odd, w_scale=s4),
                dict(codes=c8.view(torch.int8)), dict(codes=c8.cpu()),
                dict(codes=c8.float()), dict(codes=c4),      # scale: fp8's
                dict(w_scale=s4), dict(w_scale=s8[:128]),
                dict(w_scale=s8.double()), dict(w_scale=s8.cpu()),
                dict(codes=c4, w_scale=s4[:, :4].contiguous()),
                dict(codes=c4, w_scale=s4.t().contiguous().t()),
                dict(x=rnd(70, 256, dtype=F32)), dict(x=rnd(70, 512)[:, ::2]),
                dict(tile_n=16), dict(tile_n=256), dict(tile_n=-1),
                dict(act="relu"), dict(bias=rnd(128)),
                dict(residual=rnd(69, 136))):
        kw = dict(x=rnd(70, 256), codes=c8, w_scale=s8)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="linear_codes"):
            ext.linear_codes(**kw)
    torch.cuda.synchronize()  # nothing was left in flight to fail later
    x65 = rnd(65, 256)  # N = 24: the op still computes the twin
    assert torch.equal(decode_linear(x65, c4[:24], weight_scale=s4[:24]),
                       ref.decode_linear_mxfp4(x65, c4[:24], s4[:24]))
    assert torch.equal(decode_linear(x65, c8[:24], weight_scale=s8[:24]),
                       ref.decode_linear_fp8(x65, c8[:24], s8[:24]))


@pytest.mark.parametrize("wd", FMTS)
def test_captured_equals_eager_at_batch_65(gpt, wd, monkeypatch):  # noqa: F811
    calls = {}
    ext = hip_ext()
    from paddlefleetx_amd.ops import functional
    real = functional.hip_ext

    class Counting:
        def __getattr__(self, name):
            calls[name] = calls.get(name, 0) + 1
            return getattr(ext, name)

    monkeypatch.setattr(functional, "hip_ext", lambda: Counting())
    cfg = dict(_cfg("bf16"), decode_weight_dtype=wd)
    eager = GPTForGeneration(gpt, cfg)
    captured = GPTForGeneration(gpt, dict(cfg, capture_decode=True))
    ids = _prompt(65, 3)
    e1 = _generate(eager, ids, 21)
    # qkv, out_proj, ffn_up, ffn_down of every layer and the logits all have
    # N >= 128: one call each per decode step, none to the M <= 64 kernels
    assert calls.get("linear_codes", 0) == \
        (NEW - 1) * (4 * len(gpt.layers) + 1)
    assert not [k for k in calls if k.startswith("decode_linear")]
    monkeypatch.setattr(functional, "hip_ext", real)
    _assert_same(_generate(captured, ids, 21), e1)
    ids2 = _prompt(65, 4)  # a second prompt replays the same graph
    _assert_same(_generate(captured, ids2, 22), _generate(eager, ids2, 22))
