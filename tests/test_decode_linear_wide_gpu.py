"""GPU: the wide decode_linear kernel (csrc/decode_linear_wide.hip, 17 to 64
rows, bf16 weights or fp8 codes) against float64, every instance, its
masking, isolation, determinism and refusals, and batches past 16 on the tiny
GPT of test_decode_linear_gpu.py.

Accuracy bounds: the siblings', unchanged (derivations in
test_decode_linear_gpu.py and test_decode_linear_fp8_gpu.py), with
r = act((x W^T)(scale) + b) + res in float64 from the same bf16 inputs (fp8:
the same codes and scales) and S the same expression over absolute values:

    bf16   |y - r| <= 2^-8 |r| + 2 K 2^-24 S + 2^-126
    fp8    |y - r| <= 2^-8 |r| + (2 K + 2) 2^-24 S + 2^-126

plus FP32_TOL["bg.y"] with gelu.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_decode_linear_gpu import (EPILOGUES, NEW, _assert_same, _cfg,
                                    _gelu64, _generate, _one_step, _prompt,
                                    gpt)  # noqa: F401  (gpt is a fixture)
from test_ops_edges_gpu import FP32_TOL

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_linear, hip_ext
from paddlefleetx_amd.parallel.env import init_dist_env

DEV = "cuda:0"
BF16, F64, F32 = torch.bfloat16, torch.float64, torch.float32
FP8 = torch.float8_e4m3fn

# M: one row in a new column tile, or a full one. (24, 64): one and a half
# row tiles, a single fp8 k-step, more waves than k-steps. (136, 192):
# several workgroups, a partial last one. (2048, 2112): 33 fp8 / 66 bf16
# k-steps, uneven over 4 or 8 waves. (50304, 128): short K, a large grid.
MS = [17, 32, 33, 48, 49, 64]
CASES = [(n, k, m) for (n, k) in [(24, 64), (136, 192), (2048, 2112)]
         for m in MS] + [(50304, 128, 17), (50304, 128, 64)]
EPS = ["none", "bias_gelu", "bias_res"]
VARIANTS = [(rows, waves, nt) for rows in (8, 16, 32, 64)
            for waves in (4, 8) for nt in (0, 1)]

_INPUTS = {}
_REFS = {}


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


def _inputs(N, K):
    """64 rows of x, W, its codes and scales, bias and residual for one
    (N, K); smaller M are leading-row slices."""
    if (N, K) not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * N + K)
        x = torch.randn(64, K, generator=g).to(BF16).to(DEV)
        w = (torch.randn(N, K, generator=g) * 0.05).to(BF16).to(DEV)
        b = torch.randn(N, generator=g).to(BF16).to(DEV)
        r = torch.randn(64, N, generator=g).to(BF16).to(DEV)
        _INPUTS[(N, K)] = (x, w, b, r) + ref.quantize_weight_rows(w)
    return _INPUTS[(N, K)]


def _reference(N, K, ep, fp8):
    """float64 (r, S) for all 64 rows, computed once and never modified."""
    key = (N, K, ep, fp8)
    if key not in _REFS:
        x, w, b, r, c, sc = _inputs(N, K)
        bias, act, res = EPILOGUES[ep]
        w64 = c.float().to(F64) if fp8 else w.to(F64)
        y = x.to(F64) @ w64.t()
        s = x.to(F64).abs() @ w64.abs().t()
        if fp8:
            y, s = y * sc.to(F64), s * sc.to(F64)
        if bias:
            y = y + b.to(F64)
            s = s + b.to(F64).abs()
        if act == "gelu":
            y = _gelu64(y)
        if res:
            y = y + r.to(F64)
            s = s + r.to(F64).abs()
        _REFS[key] = (y, s)
    return _REFS[key]


def _check(got, N, K, M, ep, fp8, what):
    want, s = (t[:M] for t in _reference(N, K, ep, fp8))
    assert got.dtype == BF16 and got.shape == want.shape, what
    bound = 2.0 ** -8 * want.abs() \
        + (2 * K + (2 if fp8 else 0)) * 2.0 ** -24 * s + 2.0 ** -126
    if EPILOGUES[ep][1] == "gelu":
        rtol, atol = FP32_TOL["bg.y"]
        bound = bound + atol + rtol * want.abs()
    err = (got.to(F64) - want).abs()
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max())
    print(f"\n[decode_linear_wide] {'fp8' if fp8 else 'bf16'} {N}x{K} M={M} "
          f"{ep} {what}: worst err/bound = {ratio:.3g}", end="")
    assert ratio <= 1.0, f"{what}: {ratio:.3g} x bound"


def _args(N, K, M, ep, fp8):
    """(x, weight, w_scale, bias, residual, act) of the binding"""
    x, w, b, r, c, sc = _inputs(N, K)
    bias, act, res = EPILOGUES[ep]
    return (x[:M], c if fp8 else w, sc if fp8 else None, b if bias else None,
            r[:M] if res else None, act or "none")


def _op(x, w, s, b, r, act):
    return decode_linear(x, w, b, r, act, weight_scale=s)


@pytest.mark.parametrize("ep", EPS)
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("N,K,M", CASES)
def test_accuracy_against_float64(N, K, M, fp8, ep):
    args = _args(N, K, M, ep, fp8)
    direct = hip_ext().decode_linear_wide(*args)
    _check(direct, N, K, M, ep, fp8, "auto")
    # the op takes the kernel: same bits as the binding called directly
    # (bf16 weights without an epilogue stay on the library GEMM)
    if fp8 or ep != "none":
        assert torch.equal(_op(*args), direct)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("N,K,M", [(136, 192, 17), (136, 192, 33),
                                   (136, 192, 64), (2048, 2112, 64)])
def test_every_kernel_instance_is_accurate(N, K, M, fp8):
    """The automatic choice reaches few (rows, waves, nt, MT) instances on
    these shapes; the overrides reach all of them."""
    args = _args(N, K, M, "bias_res", fp8)
    for v in VARIANTS:
        got = hip_ext().decode_linear_wide(*args, *v)
        _check(got, N, K, M, "bias_res", fp8, f"rows/waves/nt={v}")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("ep", ["bias_gelu", "bias_res"])
@pytest.mark.parametrize("M", [17, 49])
def test_rows_past_m_and_n_are_never_read(M, ep, fp8):
    """Rows of x past M and of W past N are NaN (codes: byte 0x7f, the e4m3fn
    NaN, with NaN scales): none of it reaches the result, in any instance
    (64-row workgroups reach row N + 63)."""
    N, K = 136, 192
    x, w, sc, b, r, act = _args(N, K, M, ep, fp8)
    xbuf = torch.full((80, K), float("nan"), dtype=BF16, device=DEV)
    xbuf[:M] = x
    if fp8:
        wbuf = torch.full((N + 72, K), 0x7f, dtype=torch.uint8, device=DEV)
        wbuf[:N] = w.view(torch.uint8)
        wbuf = wbuf.view(FP8)
        sbuf = torch.full((N + 72,), float("nan"), dtype=F32, device=DEV)
        sbuf[:N] = sc
        sc2 = sbuf[:N]
    else:
        wbuf = torch.full((N + 72, K), float("nan"), dtype=BF16, device=DEV)
        wbuf[:N] = w
        sc2 = None
    for v in [()] + VARIANTS:
        got = hip_ext().decode_linear_wide(xbuf[:M], wbuf[:N], sc2, b, r,
                                           act, *v)
        clean = hip_ext().decode_linear_wide(x, w, sc, b, r, act, *v)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, clean), v
    _check(got, N, K, M, ep, fp8, "masked")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("N,K", [(24, 64), (136, 192)])
@pytest.mark.parametrize("M", [17, 33])
def test_rows_are_isolated(N, K, M, fp8):
    """An inf in the first row, then in the last (alone in its column tile):
    every other row keeps its bits."""
    x, *rest = _args(N, K, M, "bias_res", fp8)
    clean = _op(x, *rest)
    for hit in (0, M - 1):
        bad = x.clone()
        bad[hit, K // 2 + 3] = float("inf")
        got = _op(bad, *rest)
        keep = torch.arange(M, device=DEV) != hit
        assert torch.equal(got[keep], clean[keep])
        assert not bool(torch.isfinite(got[hit]).any())


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("N,K,M", [(24, 64, 17), (2048, 2112, 49),
                                   (50304, 128, 64)])
def test_two_calls_are_bitwise_equal(N, K, M, fp8):
    args = _args(N, K, M, "bias_gelu", fp8)
    assert torch.equal(_op(*args), _op(*args))


def test_binding_refuses_and_op_falls_back():
    g = torch.Generator().manual_seed(3)
    ext = hip_ext()

    def rnd(*shape, dtype=BF16):
        return (torch.randn(*shape, generator=g) * 0.1).to(dtype).to(DEV)

    x, w = rnd(20, 64), rnd(24, 64)
    c, s = ref.quantize_weight_rows(w)
    c96, s96 = ref.quantize_weight_rows(rnd(24, 96))
    torch.cuda.synchronize()
    for bad in (dict(x=rnd(16, 64)), dict(x=rnd(65, 64)),        # M
                dict(x=rnd(20, 96), weight=c96, w_scale=s96),    # fp8 K = 96
                dict(x=rnd(20, 40), weight=rnd(24, 40)),         # bf16 K = 40
                dict(weight=rnd(20, 64)),                        # N = 20
                dict(weight=rnd(24, 128)[:, ::2]),               # strided
                dict(x=rnd(20, 64, dtype=F32)),                  # fp32 x
                dict(rows=4), dict(rows=128), dict(waves=2),
                dict(nontemporal=2), dict(act="relu"),
                dict(bias=rnd(16)), dict(residual=rnd(16, 24)),
                dict(w_scale=s),                   # a scale with bf16 weights
                dict(weight=c),                    # codes without a scale
                dict(weight=c, w_scale=s[:16].contiguous()),
                dict(weight=c, w_scale=s.double()),
                dict(x=x.cpu(), weight=w.cpu())):
        kw = dict(x=x, weight=w)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="decode_linear_wide"):
            ext.decode_linear_wide(**kw)
    torch.cuda.synchronize()  # nothing was left in flight to fail later
    # M = 65: the op still computes the twin's expression (the bound of
    # test_decode_linear_fp8_gpu.py for two runs of the library's fp32 sum)
    x65 = rnd(65, 64)
    got, want = decode_linear(x65, c, weight_scale=s), \
        ref.decode_linear_fp8(x65, c, s)
    assert got.shape == want.shape and got.dtype == want.dtype
    mag = (x65.to(F64).abs() @ c.float().to(F64).abs().t()) * s.to(F64)
    bound = 2.0 ** -8 * mag + 2 * 64 * 2.0 ** -23 * mag + 2.0 ** -126
    assert bool(((got.to(F64) - want.to(F64)).abs() <= bound).all())


# ---------------------------------------------------------------------------
# model level: the tiny GPT of test_decode_linear_gpu.py at batches past 16
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("wdtype", ["fp8", "bf16"])
def test_captured_equals_eager_at_batch_17(gpt, wdtype, monkeypatch):  # noqa: F811
    calls = []
    ext = hip_ext()
    from paddlefleetx_amd.ops import functional
    real = functional.hip_ext

    class Counting:
        def __getattr__(self, name):
            if name == "decode_linear_wide":
                calls.append(1)
            return getattr(ext, name)

    kw = dict(decode_weight_dtype="fp8") if wdtype == "fp8" else {}
    monkeypatch.setattr(functional, "hip_ext", lambda: Counting())
    eager = GPTForGeneration(gpt, _cfg("bf16", **kw))
    captured = GPTForGeneration(gpt, _cfg("bf16", capture_decode=True, **kw))
    ids = _prompt(17, 3)
    e1 = _generate(eager, ids, 21)
    # the wide kernel ran: 4 per layer + the logits, every decode step (the
    # bf16 logits, a bare matmul, stay on the library GEMM)
    assert len(calls) == \
        (NEW - 1) * (4 * len(gpt.layers) + (wdtype == "fp8"))
    monkeypatch.setattr(functional, "hip_ext", real)
    _assert_same(_generate(captured, ids, 21), e1)
    # a second prompt replays the same graph
    ids2 = _prompt(17, 4)
    _assert_same(_generate(captured, ids2, 22), _generate(eager, ids2, 22))


def test_teacher_forced_step_at_batch_20(gpt):  # noqa: F811
    import copy
    cfg = dict(static_kv_cache=True, kv_cache_dtype="bf16", max_dec_len=2)
    gen_off = GPTForGeneration(gpt, cfg)
    gen_on = GPTForGeneration(gpt, dict(cfg, fused_decode_linear=True))
    gpt32 = copy.deepcopy(gpt).float()
    for layer in gpt32.layers:
        layer.attn.fused_attn = False  # the flash kernel is bf16 only
    ids = _prompt(20, 7)
    tok = _prompt(20, 8)[:, :1].contiguous()
    want = _one_step(gen_off, gpt32, ids, tok)
    e_off = float((_one_step(gen_off, gpt, ids, tok) - want).abs().max())
    h_on = _one_step(gen_on, gpt, ids, tok)
    e_on = float((h_on - want).abs().max())
    print(f"\n[decode_linear_wide] step: max-abs error vs fp32 reference "
          f"flag on {e_on:.3e}, flag off {e_off:.3e}", end="")
    assert e_off > 0 and torch.isfinite(h_on).all()
    assert e_on <= 2 * e_off, (e_on, e_off)
