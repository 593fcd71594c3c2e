"""GPU: fp8 KV cache kernels (csrc/decode_attention_fp8.hip) against their
fp32 reference twins on identical code bytes, plus the StaticKVCache
kv_dtype="fp8" model and generation paths."""

import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import (decode_attention, hip_ext,
                                  kv_cache_store_fp8)
from paddlefleetx_amd.parallel.env import init_dist_env
from tests.test_decode_attention_fp8_cpu import (
    FP8, NAN_CODE, N_DEC, P_LEN, fp8_cache, half_ulp_excess,
    model_reference_errors, representable_rows, teacher_forced_error)

H, SMAX = 2, 320
# The kernel as built: a lane group steps 32 rows at D=128 and 64 at D=64,
# a block iteration covers 128 / 256 positions, and with max_seq_len = SMAX
# a split chunk is 160 positions for 2 splits and 64 for 5. Both sides of
# each of those, the empty cache, one row, and the last slot of the buffer.
LENS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161,
        255, 256, 257, 319]
B = len(LENS)
DS = [64, 128]
SPLITS = [0, 1, 2, 5]  # 5: the short rows own empty splits
BF = torch.bfloat16
ONE_CODE = 0x38  # e4m3 1.0


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lens(dev):
    return torch.tensor(LENS, dtype=torch.int32, device=dev)


def _poison_tail(codes, scale):
    for b, L in enumerate(LENS):
        codes.view(torch.uint8)[b, :, L:] = NAN_CODE
        scale[b, :, L:] = float("nan")


def _u8(t):
    return t.view(torch.uint8)


@functools.lru_cache(maxsize=None)
def _case(D, amp, representable_new=False):
    """CPU tensors, built once per case and never modified: bf16 qkv, fp8
    caches quantised by the twin's quantiser with a NaN-code / NaN-scale
    tail, and what the twin returns and leaves in the caches."""
    g = torch.Generator().manual_seed(200 + D)
    qkv = torch.randn(B, 1, H, 3, D, generator=g)
    k = torch.randn(B, H, SMAX, D, generator=g) * amp
    v = torch.randn(B, H, SMAX, D, generator=g)
    qkv[:, :, :, :2] *= amp
    qkv = qkv.to(BF)
    if representable_new:
        qkv[:, :, :, 1:] = representable_rows((B, 1, H, 2, D), seed=D)
    kc, ks = ref.quantize_kv_rows(k.to(BF))
    vc, vs = ref.quantize_kv_rows(v.to(BF))
    kc, ks, vc, vs = kc.clone(), ks.clone(), vc.clone(), vs.clone()
    _poison_tail(kc, ks)
    _poison_tail(vc, vs)
    scale = 1.0 / math.sqrt(D)
    after = [t.clone() for t in (kc, ks, vc, vs)]
    want = ref.decode_attention_fp8(
        qkv.float(), after[0], after[2], after[1], after[3],
        torch.tensor(LENS, dtype=torch.int32), scale)
    return qkv, (kc, ks, vc, vs), tuple(after), scale, want


def _run(dev, case, splits):
    qkv, before, _, scale, _ = case
    qkv = qkv.to(dev)
    kc, ks, vc, vs = (t.to(dev) for t in before)
    lens = _lens(dev)
    out = decode_attention(qkv, kc, vc, lens, scale=scale, max_seq_len=SMAX,
                           num_splits=splits, k_scale=ks, v_scale=vs)
    assert torch.equal(lens, _lens(dev))
    return out.cpu(), tuple(t.cpu() for t in (kc, ks, vc, vs))


def _assert_rest_unchanged(got, before):
    """Everything but slot L of every row is bitwise what it was."""
    for new, old in zip(got, before):
        as_int = _u8 if new.dtype == FP8 else (lambda t: t.view(torch.int32))
        new, old = as_int(new).clone(), as_int(old).clone()
        for b, L in enumerate(LENS):
            new[b, :, L] = 0
            old[b, :, L] = 0
        assert torch.equal(new, old)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("D", DS)
def test_position_coverage_probe_fp8(dev, D, splits):
    """K codes 0 (scale 1) give every valid position weight 1/(L+1); channel
    d of launch r carries a one-hot V (code 1.0, scale 1) at position
    r*D + d, so out[d]*(L+1) reads how many times that position was
    counted: 1 exactly. Position L comes from qkv, not the cache; from L on
    the cache holds NaN codes and NaN scales."""
    lens = _lens(dev)
    Lp1 = (lens + 1).float()[:, None, None]  # [B, 1, 1]
    lens_col = lens.long()[:, None]          # [B, 1]
    launches = (max(LENS) + 1 + D - 1) // D
    for r in range(launches):
        pos = (torch.arange(D, device=dev) + r * D)[None, :]  # [1, D]
        in_cache = (pos < lens_col) & (pos < SMAX)            # [B, D]
        qkv = torch.zeros(B, 1, H, 3, D, device=dev, dtype=BF)
        qkv[:, :, :, 0] = 0.5  # q is irrelevant when K = 0
        qkv[:, 0, :, 2] = (pos == lens_col).to(BF)[:, None, :]
        kc = torch.zeros(B, H, SMAX, D, device=dev, dtype=torch.uint8)
        vc = torch.zeros(B, H, SMAX, D, device=dev, dtype=torch.uint8)
        bi, di = torch.nonzero(in_cache, as_tuple=True)
        vc[bi, :, di + r * D, di] = ONE_CODE
        ks = torch.ones(B, H, SMAX, device=dev)
        vs = torch.ones(B, H, SMAX, device=dev)
        kc, vc = kc.view(FP8), vc.view(FP8)
        _poison_tail(kc, ks)
        _poison_tail(vc, vs)
        expect = (pos <= lens_col).float()[:, None, :].expand(B, H, D)
        out = decode_attention(qkv, kc, vc, lens, max_seq_len=SMAX,
                               num_splits=splits, k_scale=ks, v_scale=vs)
        counted = out.float().view(B, H, D) * Lp1
        err = (counted - expect).abs().max().item()
        print(f"D={D} splits={splits} launch={r} max|count-expect|={err:.4f}")
        assert err <= 2e-2, (r, err)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("D", DS)
def test_numerics_on_shared_codes(dev, D, splits):
    case = _case(D, 1.0)
    qkv, _, _, _, want = case
    out, _ = _run(dev, case, splits)
    assert out.shape == (B, 1, H * D) and out.dtype == BF
    assert torch.isfinite(out.float()).all()
    err = (out.float() - want).abs().max().item()
    print(f"D={D} splits={splits} max|out-twin|={err:.5f}")
    assert torch.allclose(out.float(), want, atol=3e-2, rtol=3e-2), err
    # L = 0: softmax over the single, unquantised new token is exactly v_new
    assert torch.equal(out[0, 0].view(torch.int16),
                       qkv[0, 0, :, 2].reshape(-1).view(torch.int16))


@pytest.mark.parametrize("splits", [1, 5])
@pytest.mark.parametrize("D", DS)
def test_large_scores_fp8(dev, D, splits):
    """Raw scores beyond +-60: the online-max rescale inside a split and
    the merge across splits, with scores that carry the row scale."""
    case = _case(D, 5.5)
    qkv, (kc, ks, _, _), _, scale, want = case
    kf = torch.nan_to_num(ref.dequantize_kv_rows(kc, ks))
    s = torch.einsum("bhd,bhsd->bhs", qkv[:, 0, :, 0].float(), kf) * scale
    assert s.abs().max() > 60.0
    out, _ = _run(dev, case, splits)
    assert torch.isfinite(out.float()).all()
    err = (out.float() - want).abs().max().item()
    print(f"D={D} splits={splits} large-score max|out-twin|={err:.5f}")
    assert torch.allclose(out.float(), want, atol=3e-2, rtol=3e-2), err


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("D", DS)
def test_append_representable_is_bitwise(dev, D, splits):
    case = _case(D, 1.0, True)
    _, before, after, _, _ = case
    _, got = _run(dev, case, splits)
    # the whole caches, slot L included, are the twin's bitwise
    for new, exp in zip(got, after):
        if new.dtype == FP8:
            assert torch.equal(_u8(new), _u8(exp))
        else:
            assert torch.equal(new.view(torch.int32), exp.view(torch.int32))
    _assert_rest_unchanged(got, before)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("D", DS)
def test_append_random_scale_bitwise_codes_in_bound(dev, D, splits):
    case = _case(D, 1.0)
    qkv, before, after, _, _ = case
    _, got = _run(dev, case, splits)
    _assert_rest_unchanged(got, before)
    rows = torch.arange(B)
    at = torch.tensor(LENS)
    differ = 0
    for which, ci, si in ((1, 0, 1), (2, 2, 3)):
        new = qkv[:, 0, :, which].float()              # [B, H, D]
        codes, sc = got[ci][rows, :, at], got[si][rows, :, at]
        assert torch.equal(sc.view(torch.int32),
                           after[si][rows, :, at].view(torch.int32))
        assert not torch.isnan(codes.float()).any()
        ratio = half_ulp_excess(new, codes, sc)
        assert ratio <= 1.0, ratio
        differ += (_u8(codes) != _u8(after[ci][rows, :, at])).sum().item()
    print(f"D={D} splits={splits}: {differ} of {2 * B * H * D} appended code "
          f"bytes differ from torch's cast (informational)")


@pytest.mark.parametrize("S", [1, 5, 17])
@pytest.mark.parametrize("D", DS)
def test_prefill_store(dev, D, S):
    Bp, Smax = 2, 32
    g = torch.Generator().manual_seed(300 + D + S)
    rand = (torch.randn(Bp, S, H, 3, D, generator=g)
            * torch.logspace(-2, 1, S)[None, :, None, None, None]).to(BF)
    exact = rand.clone()
    exact[:, :, :, 1:] = representable_rows((Bp, S, H, 2, D), seed=S)
    for name, qkv in (("random", rand), ("representable", exact)):
        want = (torch.full((Bp, H, Smax, D), NAN_CODE,
                           dtype=torch.uint8).view(FP8),
                torch.full((Bp, H, Smax), float("nan")),
                torch.full((Bp, H, Smax, D), NAN_CODE,
                           dtype=torch.uint8).view(FP8),
                torch.full((Bp, H, Smax), float("nan")))
        got = tuple(t.clone().to(dev) for t in want)
        ref.kv_store_fp8(qkv.float(), want[0], want[2], want[1], want[3])
        kv_cache_store_fp8(qkv.to(dev), got[0], got[2], got[1], got[3])
        got = tuple(t.cpu() for t in got)
        differ = 0
        for which, ci, si in ((1, 0, 1), (2, 2, 3)):
            # scales bitwise, NaN tail included
            assert torch.equal(got[si].view(torch.int32),
                               want[si].view(torch.int32))
            assert (_u8(got[ci])[:, :, S:] == NAN_CODE).all()
            codes = got[ci][:, :, :S]
            x = qkv[:, :, :, which].transpose(1, 2).float()
            assert not torch.isnan(codes.float()).any()
            ratio = half_ulp_excess(x, codes, got[si][:, :, :S])
            assert ratio <= 1.0, (name, ratio)
            differ += (_u8(got[ci]) != _u8(want[ci])).sum().item()
        print(f"D={D} S={S} {name}: {differ} code bytes differ from the twin")
        if name == "representable":
            assert differ == 0


def test_argument_errors_fp8(dev):
    """Host checks fire before any launch."""
    ext = hip_ext()
    D = 64
    lens = torch.zeros(2, dtype=torch.int32, device=dev)

    def mk(dtype=BF, cdtype=FP8, sdtype=torch.float32, d=D, smax_s=16, S=1):
        return [torch.zeros(2, S, H, 3, d, device=dev, dtype=dtype),
                torch.zeros(2, H, 16, d, device=dev).to(cdtype),
                torch.zeros(2, H, 16, d, device=dev).to(cdtype),
                torch.ones(2, H, smax_s, device=dev, dtype=sdtype),
                torch.ones(2, H, smax_s, device=dev, dtype=sdtype)]

    fn = ext.decode_attn_fp8
    with pytest.raises(RuntimeError, match="bf16"):
        fn(*mk(dtype=torch.float16), lens, 0.125, 16, 0)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        fn(*mk(cdtype=BF), lens, 0.125, 16, 0)
    with pytest.raises(RuntimeError, match="fp32"):
        fn(*mk(sdtype=torch.float16), lens, 0.125, 16, 0)
    with pytest.raises(RuntimeError, match="k_scale and v_scale"):
        fn(*mk(smax_s=15), lens, 0.125, 16, 0)
    with pytest.raises(RuntimeError, match="head_dim"):
        fn(*mk(d=32), lens, 0.125, 16, 0)
    with pytest.raises(RuntimeError, match="max_seq_len"):
        fn(*mk(), lens, 0.125, 17, 0)
    with pytest.raises(RuntimeError, match="max_seq_len"):
        fn(*mk(), lens, 0.125, 0, 0)
    with pytest.raises(RuntimeError, match="num_splits"):
        fn(*mk(), lens, 0.125, 16, 33)
    with pytest.raises(RuntimeError, match="int32"):
        fn(*mk(), lens.long(), 0.125, 16, 0)
    with pytest.raises(RuntimeError, match=r"\[B, 1, h, 3, D\]"):
        fn(*mk(S=2), lens, 0.125, 16, 0)
    with pytest.raises(RuntimeError, match="contiguous"):
        a = mk()
        a[1] = a[1].transpose(1, 2).contiguous().transpose(1, 2)
        fn(*a, lens, 0.125, 16, 0)
    with pytest.raises(RuntimeError, match="contiguous"):
        a = mk()
        a[3] = a[3].transpose(1, 2).contiguous().transpose(1, 2)
        fn(*a, lens, 0.125, 16, 0)

    st = ext.kv_store_fp8
    with pytest.raises(RuntimeError, match="S must be <= Smax"):
        st(*mk(S=17))
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        st(*mk(cdtype=BF, S=4))
    with pytest.raises(RuntimeError, match="k_scale and v_scale"):
        st(*mk(smax_s=15, S=4))
    with pytest.raises(RuntimeError, match="head_dim"):
        st(*mk(d=32, S=4))
    with pytest.raises(RuntimeError, match="contiguous"):
        a = mk(S=4)
        a[0] = a[0].transpose(1, 2).contiguous().transpose(1, 2)
        st(*a)


def test_model_fp8_cache_error_inequality_gpu(dev):
    """The inequality of the CPU test with e_fp8 from the bf16 model on the
    GPU over the HIP fp8 path; e_old and e_sim come from references."""
    gpt16, ids, pos, want, e_old, e_sim = model_reference_errors()
    gpt = copy.deepcopy(gpt16).to(dev)
    cache = fp8_cache(dev)
    e_fp8 = teacher_forced_error(gpt, want, ids, pos, cache)
    print(f"e_old={e_old:.5f} e_sim={e_sim:.5f} e_fp8={e_fp8:.5f} "
          f"bound={1.5 * e_sim + 2.0 * e_old:.5f}")
    assert cache.max_len == P_LEN + N_DEC
    assert cache.k[0].dtype == FP8 and cache.k[0].is_cuda
    assert e_old > 0.0 and e_sim > 0.0
    assert e_fp8 <= 1.5 * e_sim + 2.0 * e_old, (e_fp8, e_sim, e_old)


def test_generation_fp8_cache(dev):
    gpt16 = model_reference_errors()[0]
    gpt = copy.deepcopy(gpt16).to(dev)
    cfg = {"max_dec_len": 8, "min_dec_len": 8, "eos_token_id": 511,
           "decoding_strategy": "greedy_search", "static_kv_cache": True,
           "kv_cache_dtype": "fp8"}
    gen = GPTForGeneration(gpt, cfg)
    torch.manual_seed(3)
    ids = torch.randint(0, 511, (2, 5), device=dev)
    out1, out2 = gen(ids), gen(ids)
    assert out1.shape == (2, 8)
    assert torch.equal(out1, out2)
    assert (out1 >= 0).all() and (out1 < 512).all()
