"""GPU: fused decode attention (csrc/decode_attention.hip) against its fp32
reference twin, plus the StaticKVCache model and generation paths."""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import GPTModel, StaticKVCache
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_attention, hip_ext
from paddlefleetx_amd.parallel.env import init_dist_env

H, SMAX, B = 2, 320, 8
# empty cache, one row, both sides of the 64- and 256-position chunk and
# split boundaries, and the last slot of the buffer
LENS = [0, 1, 63, 64, 65, 255, 256, 318]
DS = [64, 128]
SPLITS = [0, 1, 2, 5]  # 5: the short rows own empty splits
BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lens(dev):
    return torch.tensor(LENS, dtype=torch.int32, device=dev)


def _poison_tail(cache, value):
    for b, L in enumerate(LENS):
        cache[b, :, L:] = value


@functools.lru_cache(maxsize=None)
def _random_case(D, amp):
    """bf16 inputs with a NaN tail and the fp32 reference output, computed
    once per (D, amplitude) and shared; callers clone the caches."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(100 + D)
    qkv = (torch.randn(B, 1, H, 3, D, generator=g) * 1.0).to(dev)
    k = torch.randn(B, H, SMAX, D, generator=g).to(dev)
    v = torch.randn(B, H, SMAX, D, generator=g).to(dev)
    qkv[:, :, :, :2] *= amp
    k *= amp
    qkv, k, v = qkv.to(BF), k.to(BF), v.to(BF)
    _poison_tail(k, float("nan"))
    _poison_tail(v, float("nan"))
    scale = 1.0 / math.sqrt(D)
    want = ref.decode_attention(qkv.float(), k.float(), v.float(),
                                _lens(dev), scale)
    return qkv, k, v, scale, want


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("D", DS)
def test_position_coverage_probe(dev, D, splits):
    """K = 0 gives every valid position weight 1/(L+1); channel d of launch
    r carries a one-hot V at position r*D + d, so out[d]*(L+1) reads how
    many times that position was counted: 1 exactly (0 dropped, 2 doubled).
    Position L comes from qkv, not the cache; past L the cache holds 1000."""
    lens = _lens(dev)
    Lp1 = (lens + 1).float()[:, None, None]  # [B, 1, 1]
    launches = (max(LENS) + 1 + D - 1) // D
    for r in range(launches):
        pos = torch.arange(D, device=dev) + r * D  # p_d
        qkv = torch.zeros(B, 1, H, 3, D, device=dev, dtype=BF)
        qkv[:, :, :, 0] = 0.5  # q is irrelevant when K = 0
        k = torch.zeros(B, H, SMAX, D, device=dev, dtype=BF)
        v = torch.zeros(B, H, SMAX, D, device=dev, dtype=BF)
        expect = torch.zeros(B, H, D, device=dev)
        for b, L in enumerate(LENS):
            in_cache = pos < L
            v[b, :, pos[in_cache], torch.nonzero(in_cache).flatten()] = 1.0
            is_new = pos == L
            qkv[b, 0, :, 2, is_new] = 1.0
            expect[b, :, pos <= L] = 1.0
        _poison_tail(k, 1000.0)
        _poison_tail(v, 1000.0)
        out = decode_attention(qkv, k, v, lens, max_seq_len=SMAX,
                               num_splits=splits)
        counted = out.float().view(B, H, D) * Lp1
        err = (counted - expect).abs().max().item()
        print(f"D={D} splits={splits} launch={r} max|count-expect|={err:.4f}")
        assert err <= 2e-2, (r, err)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("D", DS)
def test_random_numerics_and_inplace_append(dev, D, splits):
    qkv, k0, v0, scale, want = _random_case(D, 1.0)
    k, v = k0.clone(), v0.clone()
    lens = _lens(dev)
    out = decode_attention(qkv, k, v, lens, scale=scale, max_seq_len=SMAX,
                           num_splits=splits)
    assert out.shape == (B, 1, H * D) and out.dtype == BF
    assert torch.isfinite(out.float()).all()
    err = (out.float() - want).abs().max().item()
    print(f"D={D} splits={splits} max|out-ref|={err:.5f}")
    assert torch.allclose(out.float(), want, atol=3e-2, rtol=3e-2), err
    # L = 0: softmax over the single new token is exactly v_new
    assert torch.equal(out[0, 0].view(torch.int16),
                       qkv[0, 0, :, 2].reshape(-1).view(torch.int16))
    # in-place append: slot L holds the new K/V bitwise, every other
    # element (NaN tail included) is bitwise unchanged; lens untouched
    assert torch.equal(lens, _lens(dev))
    for new, old, which in ((k, k0, 1), (v, v0, 2)):
        new_i, exp_i = new.view(torch.int16), old.clone().view(torch.int16)
        for b, L in enumerate(LENS):
            exp_i[b, :, L] = qkv[b, 0, :, which].view(torch.int16)
        assert torch.equal(new_i, exp_i)


@pytest.mark.parametrize("splits", [1, 5])
@pytest.mark.parametrize("D", DS)
def test_large_scores(dev, D, splits):
    """Raw scores of about +-80 (std ~30): exercises the online-max rescale
    inside a split and the merge across splits."""
    qkv, k0, v0, scale, want = _random_case(D, 5.5)
    kf = torch.nan_to_num(k0.float())
    s = torch.einsum("bhd,bhsd->bhs", qkv[:, 0, :, 0].float(), kf) * scale
    assert s.abs().max() > 60.0
    k, v = k0.clone(), v0.clone()
    out = decode_attention(qkv, k, v, _lens(dev), scale=scale,
                           max_seq_len=SMAX, num_splits=splits)
    assert torch.isfinite(out.float()).all()
    err = (out.float() - want).abs().max().item()
    print(f"D={D} splits={splits} large-score max|out-ref|={err:.5f}")
    assert torch.allclose(out.float(), want, atol=3e-2, rtol=3e-2), err


def test_argument_errors(dev):
    """Host checks fire before any launch."""
    fn = hip_ext().decode_attn
    D = 64
    lens = torch.zeros(2, dtype=torch.int32, device=dev)

    def mk(dtype=BF, d=D):
        return (torch.zeros(2, 1, H, 3, d, device=dev, dtype=dtype),
                torch.zeros(2, H, 16, d, device=dev, dtype=dtype),
                torch.zeros(2, H, 16, d, device=dev, dtype=dtype))

    with pytest.raises(RuntimeError, match="bf16"):
        fn(*mk(dtype=torch.float16), lens, 0.125, 16, 0)
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
    with pytest.raises(RuntimeError, match="contiguous"):
        q, k, v = mk()
        fn(q, k.transpose(1, 2).contiguous().transpose(1, 2), v, lens,
           0.125, 16, 0)


def _gpu_gpt(dev, dtype, vocab=512):
    torch.manual_seed(11)
    with torch.device(dev):
        return GPTModel(vocab_size=vocab, hidden_size=256, num_layers=2,
                        num_attention_heads=2, max_position_embeddings=64,
                        hidden_dropout_prob=0.0,
                        attention_probs_dropout_prob=0.0,
                        dtype=dtype).eval()


def test_model_static_cache_error_vs_fp32(dev):
    """Teacher-forced prefill 16 + decode 6. The tuple-cache and the static
    cache logits are both bf16 roundings of the fp32 model's logits; the
    static path may be at most 2x as far from fp32 as the tuple path."""
    P, N = 16, 6
    gpt = _gpu_gpt(dev, BF)
    gpt32 = GPTModel(vocab_size=512, hidden_size=256, num_layers=2,
                     num_attention_heads=2, max_position_embeddings=64,
                     hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0, fused_attn=False,
                     dtype=torch.float32).eval()
    gpt32.load_state_dict({n: t.float().cpu()
                           for n, t in gpt.state_dict().items()})
    torch.manual_seed(5)
    ids = torch.randint(0, 512, (2, P + N))
    pos = torch.arange(P + N).unsqueeze(0).expand(2, -1)
    with torch.no_grad():
        hid = gpt32(ids, pos)
        want = hid @ gpt32.embeddings.word_embeddings.weight.t()  # [2,S,V]
    ids, pos = ids.to(dev), pos.to(dev)
    gen = GPTForGeneration(gpt, {})
    static = StaticKVCache(2, 2, 2, P + N, 128, dtype=BF, device=dev)
    e_old = e_new = 0.0
    with torch.no_grad():
        lt, tc = gen._logits(ids[:, :P], pos[:, :P], None)
        ls, sc = gen._logits(ids[:, :P], pos[:, :P], static)
        steps = [(P - 1, lt, ls)]
        for t in range(P, P + N):
            lt, tc = gen._logits(ids[:, t:t + 1], pos[:, t:t + 1], tc)
            ls, sc = gen._logits(ids[:, t:t + 1], pos[:, t:t + 1], sc)
            steps.append((t, lt, ls))
    for t, lt, ls in steps:
        e_old = max(e_old, (lt.cpu() - want[:, t]).abs().max().item())
        e_new = max(e_new, (ls.cpu() - want[:, t]).abs().max().item())
    print(f"e_old={e_old:.5f} e_new={e_new:.5f}")
    assert static.max_len == P + N
    assert e_old > 0.0
    assert e_new <= 2.0 * e_old, (e_new, e_old)


def test_generation_static_cache(dev):
    gpt = _gpu_gpt(dev, BF)
    cfg = {"max_dec_len": 8, "min_dec_len": 8, "eos_token_id": 511,
           "decoding_strategy": "greedy_search", "static_kv_cache": True}
    gen = GPTForGeneration(gpt, cfg)
    torch.manual_seed(3)
    ids = torch.randint(0, 511, (2, 5), device=dev)
    out1, out2 = gen(ids), gen(ids)
    assert out1.shape == (2, 8)
    assert torch.equal(out1, out2)
    samp = GPTForGeneration(gpt, dict(cfg, decoding_strategy="sampling",
                                      top_p=0.9, use_topp_sampling=True))
    out3 = samp(ids)
    assert out3.shape == (2, 8)
    assert (out3 >= 0).all() and (out3 < 512).all()
