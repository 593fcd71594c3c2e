"""GPU: the fp8-weight decode_linear kernel (csrc/decode_linear_fp8.hip)
against float64, every variant, its masking, isolation, determinism and
refusals, and the fp8 decode weights on a tiny GPT.

Accuracy bound (derived, not tuned), r = act((x codes^T) scale + b) + res in
float64 from the same bf16 inputs, codes and scales,
S = (|x| |codes|^T) scale + |b| + |res|:

    |y - r| <= 2^-8 |r| + (2 K + 2) 2^-24 S + 2^-126

The codes decode exactly to bf16, so x . codes^T is the fp32 accumulation of
K exact products as in test_decode_linear_gpu.py (factor 2 for the MFMA's
internal order); +2 is the multiply by the scale; 2^-8 |r| the one rounding
to bf16. With gelu the project's fp32 bias-gelu tolerance is added.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_ops_edges_gpu import FP32_TOL

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import GPTModel, StaticKVCache
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_linear, hip_ext
from paddlefleetx_amd.parallel.env import init_dist_env

DEV = "cuda:0"
BF16, F64, F32 = torch.bfloat16, torch.float64, torch.float32
FP8 = torch.float8_e4m3fn

# (16, 64): one step. (24, 192): partial tile; 3 steps, so some waves have
# none. (136, 2112): 33 steps in uneven chunks with a partial batch; N a
# multiple of 8 but not of 16. (512, 128): many tiles, short K.
# (50304, 128): a vocabulary-sized grid.
SHAPES = [(16, 64), (24, 192), (136, 2112), (512, 128), (50304, 128)]
MS = [1, 2, 5, 16]
CASES = [(n, k, m) for (n, k) in SHAPES for m in MS] + [(2048, 8192, 16)]
# (bias, activation, residual): the five of test_decode_linear_gpu.py
EPILOGUES = {"none": (False, None, False), "bias": (True, None, False),
             "bias_gelu": (True, "gelu", False),
             "bias_res": (True, None, True), "res": (False, None, True)}
VARIANTS = [(rows, waves, nt) for rows in (8, 16, 32, 64)
            for waves in (4, 8) for nt in (0, 1)]

_INPUTS = {}
_REFS = {}


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


def _inputs(N, K):
    """16 rows of x, codes, scales, bias and residual for one (N, K);
    smaller M are leading-row slices, so every case of a shape shares one
    set."""
    if (N, K) not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * N + K)
        x = torch.randn(16, K, generator=g).to(BF16).to(DEV)
        w = (torch.randn(N, K, generator=g) * 0.05).to(BF16).to(DEV)
        b = torch.randn(N, generator=g).to(BF16).to(DEV)
        r = torch.randn(16, N, generator=g).to(BF16).to(DEV)
        c, s = ref.quantize_weight_rows(w)
        _INPUTS[(N, K)] = (x, c, s, b, r)
    return _INPUTS[(N, K)]


def _gelu64(y):
    return 0.5 * y * (1.0 + torch.tanh(
        0.7978845608028654 * (y + 0.044715 * y ** 3)))


def _reference(N, K, ep):
    """float64 (r, S) for all 16 rows of one shape and epilogue, computed
    once and never modified."""
    key = (N, K, ep)
    if key not in _REFS:
        x, c, sc, b, r = _inputs(N, K)
        bias, act, res = EPILOGUES[ep]
        c64, s64 = c.float().to(F64), sc.to(F64)
        y = (x.to(F64) @ c64.t()) * s64
        s = (x.to(F64).abs() @ c64.abs().t()) * s64
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


def _bound(want, s, K, gelu):
    bound = 2.0 ** -8 * want.abs() + (2 * K + 2) * 2.0 ** -24 * s \
        + 2.0 ** -126
    if gelu:
        rtol, atol = FP32_TOL["bg.y"]
        bound = bound + atol + rtol * want.abs()
    return bound


def _check(got, want, s, K, gelu, what):
    assert got.dtype == BF16 and got.shape == want.shape, what
    err = (got.to(F64) - want).abs()
    bound = _bound(want, s, K, gelu)
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max())
    print(f"\n[decode_linear_fp8] {what}: worst err/bound = {ratio:.3g}",
          end="")
    assert ratio <= 1.0, f"{what}: {ratio:.3g} x bound"


def _args(N, K, M, ep):
    """(x, codes, bias, residual, act, scale)"""
    x, c, s, b, r = _inputs(N, K)
    bias, act, res = EPILOGUES[ep]
    return (x[:M], c, b if bias else None, r[:M] if res else None, act, s)


def _op(x, c, b, r, act, s):
    return decode_linear(x, c, b, r, act, weight_scale=s)


@pytest.mark.parametrize("ep", list(EPILOGUES))
@pytest.mark.parametrize("N,K,M", CASES)
def test_accuracy_against_float64(N, K, M, ep):
    x, c, b, r, act, s = _args(N, K, M, ep)
    got = _op(x, c, b, r, act, s)
    want, mag = _reference(N, K, ep)
    _check(got, want[:M], mag[:M], K, act == "gelu", f"{N}x{K} M={M} {ep}")
    # the op took the kernel: same bits as the binding called directly
    direct = hip_ext().decode_linear_fp8(x, c, s, b, r, act or "none")
    assert torch.equal(got, direct)


@pytest.mark.parametrize("rows,waves,nt", VARIANTS)
@pytest.mark.parametrize("N,K,M", [(24, 192, 5), (136, 2112, 16)])
def test_every_kernel_variant_is_accurate(N, K, M, rows, waves, nt):
    """The automatic choice reaches only some (rows, waves, nt) instances on
    the shapes above; the overrides reach the others."""
    x, c, b, r, _, s = _args(N, K, M, "bias_res")
    got = hip_ext().decode_linear_fp8(x, c, s, b, r, "none", rows, waves, nt)
    want, mag = _reference(N, K, "bias_res")
    _check(got, want[:M], mag[:M], K, False,
           f"{N}x{K} M={M} rows={rows} waves={waves} nt={nt}")


@pytest.mark.parametrize("ep", ["bias_gelu", "bias_res"])
@pytest.mark.parametrize("M", MS)
def test_rows_past_m_and_n_are_never_read(M, ep):
    """Code rows past N hold byte 0x7f (the e4m3fn NaN), scales past N and
    x rows past M are NaN: none of it reaches the result."""
    N, K = 24, 192
    x, c, sc, b, r = _inputs(N, K)
    xbuf = torch.full((32, K), float("nan"), dtype=BF16, device=DEV)
    cbuf = torch.full((N + 72, K), 0x7f, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((N + 72,), float("nan"), dtype=F32, device=DEV)
    xbuf[:M] = x[:M]
    cbuf[:N] = c.view(torch.uint8)
    sbuf[:N] = sc
    bias, act, res = EPILOGUES[ep]
    rr = r[:M] if res else None
    got = _op(xbuf[:M], cbuf.view(FP8)[:N], b, rr, act, sbuf[:N])
    assert bool(torch.isfinite(got).all())
    want, mag = _reference(N, K, ep)
    _check(got, want[:M], mag[:M], K, act == "gelu", f"masked M={M} {ep}")
    assert torch.equal(got, _op(*_args(N, K, M, ep)))
    # every variant masks the same way (64-row workgroups reach row N + 63)
    for v in VARIANTS:
        gv = hip_ext().decode_linear_fp8(
            xbuf[:M], cbuf.view(FP8)[:N], sbuf[:N], b, rr, act or "none", *v)
        cv = hip_ext().decode_linear_fp8(
            x[:M], c, sc, b, rr, act or "none", *v)
        assert bool(torch.isfinite(gv).all()) and torch.equal(gv, cv), v


@pytest.mark.parametrize("N,K", [(24, 192), (136, 2112)])
@pytest.mark.parametrize("M", [2, 5, 16])
def test_rows_are_isolated(N, K, M):
    x, c, b, r, _, s = _args(N, K, M, "bias_res")
    clean = _op(x, c, b, r, None, s)
    bad = x.clone()
    bad[0, K // 2 + 3] = float("inf")
    got = _op(bad, c, b, r, None, s)
    assert torch.equal(got[1:], clean[1:])
    assert not bool(torch.isfinite(got[0]).any())


@pytest.mark.parametrize("N,K,M", [(24, 192, 5), (136, 2112, 16),
                                   (50304, 128, 2)])
def test_two_calls_are_bitwise_equal(N, K, M):
    args = _args(N, K, M, "bias_gelu")
    assert torch.equal(_op(*args), _op(*args))


def _refused(x, c, s):
    ext = hip_ext()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="decode_linear_fp8"):
        ext.decode_linear_fp8(x, c, s)
    torch.cuda.synchronize()  # and nothing was left in flight to fail later
    got = decode_linear(x, c, weight_scale=s)
    want = ref.decode_linear_fp8(x, c, s)
    assert got.shape == want.shape and got.dtype == want.dtype
    # the fallback IS the twin's expression: two fp32 sums of K products in
    # the library's order, one rounding each
    K = x.shape[1]
    mag = (x.to(F64).abs() @ c.float().to(F64).abs().t()) * s.to(F64)
    eps = 2.0 ** -8 if x.dtype == BF16 else 2.0 ** -24
    bound = eps * mag + 2 * K * 2.0 ** -23 * mag + 2.0 ** -126
    err = (got.to(F64) - want.to(F64)).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


def test_binding_refuses_and_op_falls_back():
    g = torch.Generator().manual_seed(3)

    def rnd(*shape, dtype=BF16):
        return (torch.randn(*shape, generator=g) * 0.1).to(dtype).to(DEV)

    def q(*shape):
        return ref.quantize_weight_rows(rnd(*shape))

    _refused(rnd(17, 64), *q(24, 64))                        # M = 17
    _refused(rnd(4, 96), *q(24, 96))                         # K = 96
    _refused(rnd(4, 32), *q(24, 32))                         # K = 32
    _refused(rnd(4, 64), *q(20, 64))                         # N = 20
    _refused(rnd(4, 64, dtype=F32), *q(24, 64))              # fp32 x
    c, s = q(24, 128)
    _refused(rnd(4, 64), c[:, ::2], s)                       # strided codes
    c, s = q(25, 64)
    _refused(rnd(4, 64), c.view(torch.uint8).flatten()[8:8 + 24 * 64]
             .view(FP8).view(24, 64), s[:24].contiguous())   # misaligned
    c, s = q(24, 64)
    _refused(rnd(4, 64), c, torch.stack([s, s], 1)[:, 0])    # strided scale
    ext = hip_ext()
    x = rnd(4, 64)
    for bad in (dict(bias=rnd(16)), dict(residual=rnd(4, 16)),
                dict(act="relu"), dict(bias=rnd(24).float()),
                dict(rows=4), dict(rows=128), dict(waves=2),
                dict(nontemporal=2), dict(w_scale=s.double()),
                dict(w_scale=s[:16].contiguous()), dict(w_scale=s.cpu()),
                dict(wq=c.float().to(BF16)),
                dict(wq=c.view(torch.float8_e5m2))):
        kw = dict(x=x, wq=c, w_scale=s)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="decode_linear_fp8"):
            ext.decode_linear_fp8(**kw)
    with pytest.raises(RuntimeError, match="decode_linear_fp8"):
        ext.decode_linear_fp8(x.cpu(), c.cpu(), s.cpu())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# model level: the tiny GPT of test_decode_linear_gpu.py
# ---------------------------------------------------------------------------

VOCAB, PROMPT, NEW, CAPACITY = 512, 5, 12, 24


@pytest.fixture(scope="module")
def gpt():
    torch.manual_seed(11)
    with torch.device(DEV):
        m = GPTModel(vocab_size=VOCAB, hidden_size=128, num_layers=2,
                     num_attention_heads=2, max_position_embeddings=64,
                     hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0,
                     dtype=torch.bfloat16).eval()
    # biases start at zero: make every epilogue term count
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_((torch.randn(p.shape, generator=g) * 0.1)
                       .to(p.dtype).to(DEV))
    return m


def _cfg(kv, **kw):
    return dict(max_dec_len=NEW, min_dec_len=NEW, eos_token_id=VOCAB - 1,
                static_kv_cache=True, kv_cache_dtype=kv, fused_sampling=True,
                kv_cache_capacity=CAPACITY, top_k=20, top_p=0.9,
                temperature=0.8, repetition_penalty=1.2,
                fused_decode_linear=True, decode_weight_dtype="fp8", **kw)


def _prompt(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, VOCAB - 1, (B, PROMPT), generator=g).to(DEV)


def _generate(gen, ids, seed):
    """(tokens, final lens, valid K/V [+ scales] per layer), on the CPU."""
    torch.manual_seed(seed)
    with torch.no_grad():
        out, st = gen._sample_fused(ids, return_state=True)
    cache = st["cache"]
    lens = cache.lens.cpu()
    L = int(lens.max())
    kv = []
    for bufs in (cache.k, cache.v, cache.k_scale or [], cache.v_scale or []):
        for t in bufs:
            t = t[:, :, :L]
            kv.append((t.view(torch.uint8) if t.element_size() == 1 else t)
                      .cpu().clone())
    return out.cpu(), lens, kv


def _assert_same(a, b):
    assert a[0].shape == (a[0].shape[0], NEW)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1])
    assert a[1].tolist() == [PROMPT + NEW - 1] * a[0].shape[0]
    assert len(a[2]) == len(b[2]) > 0
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_captured_equals_eager_with_fp8_weights(gpt, kv, monkeypatch):
    calls = {"decode_linear_fp8": 0, "decode_linear": 0}
    ext = hip_ext()
    from paddlefleetx_amd.ops import functional
    real = functional.hip_ext

    class Counting:
        def __getattr__(self, name):
            if name in calls:
                calls[name] += 1
            return getattr(ext, name)

    monkeypatch.setattr(functional, "hip_ext", lambda: Counting())
    eager = GPTForGeneration(gpt, _cfg(kv))
    captured = GPTForGeneration(gpt, _cfg(kv, capture_decode=True))
    ids = _prompt(2, 3)
    e1 = _generate(eager, ids, 21)
    # the fp8 kernel itself ran: 4 per layer + the logits, every decode step
    assert calls["decode_linear_fp8"] == (NEW - 1) * (4 * len(gpt.layers) + 1)
    assert calls["decode_linear"] == 0
    monkeypatch.setattr(functional, "hip_ext", real)
    c1 = _generate(captured, ids, 21)
    _assert_same(c1, e1)
    # a second prompt replays the same graph
    graph = captured._graph_state["graph"]
    ids2 = _prompt(2, 4)
    _assert_same(_generate(captured, ids2, 22), _generate(eager, ids2, 22))
    assert captured._graph_state["graph"] is graph
    # the codes are not in any checkpoint
    assert list(captured.state_dict()) == \
        list(GPTForGeneration(gpt, {}).state_dict())


def _one_step(gen, model, ids, tok, prefill_model=None):
    """Prefill with prefill_model (default: model), one forced decode token
    with model, both against one cache of gen's kind."""
    B, P = ids.shape
    cache = gen._new_static_cache(B, P + 2, ids.device)
    if model.embeddings.word_embeddings.weight.dtype != torch.bfloat16:
        # the fp32 reference model keeps an fp32 cache
        attn = model.layers[0].attn
        cache = StaticKVCache(len(model.layers), B, attn.num_heads_local,
                              P + 2, attn.head_dim, dtype=torch.float32,
                              device=ids.device)
    pos = torch.arange(P, device=ids.device).unsqueeze(0).expand(B, -1)
    with torch.no_grad():
        (prefill_model or model)(ids, pos, caches=cache, use_cache=True)
        hidden, _ = model(tok, cache.lens.long().unsqueeze(1), caches=cache,
                          use_cache=True)
    return hidden.float()


def _linear_weights(m):
    ws = []
    for layer in m.layers:
        ws += [layer.attn.qkv.weight, layer.attn.out_proj.weight,
               layer.ffn.up.weight, layer.ffn.down.weight]
    return ws


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_teacher_forced_step_is_no_worse_than_existing_path(gpt, kv):
    """Reference: the fp32 model whose decode linears hold code * scale
    (prompt processed with the unquantised fp32 weights, as the mode does).
    Off: the bf16 model with those weights rounded to bf16 on the existing
    fused path. On: the fp8 path of the unchanged bf16 model."""
    import copy
    cfg = dict(static_kv_cache=True, kv_cache_dtype=kv, max_dec_len=2,
               fused_decode_linear=True)
    gen_off = GPTForGeneration(gpt, cfg)
    gen_on = GPTForGeneration(gpt, dict(cfg, decode_weight_dtype="fp8"))
    gpt32 = copy.deepcopy(gpt).float()
    deq32 = copy.deepcopy(gpt32)
    deq16 = copy.deepcopy(gpt)
    with torch.no_grad():
        for w, w32, w16 in zip(_linear_weights(gpt), _linear_weights(deq32),
                               _linear_weights(deq16)):
            c, s = ref.quantize_weight_rows(w)
            w32.copy_(ref.dequantize_kv_rows(c, s))
            w16.copy_(ref.dequantize_kv_rows(c, s))  # rounds to bf16
    for m in (gpt32, deq32):
        for layer in m.layers:
            layer.attn.fused_attn = False  # the flash kernel is bf16 only
    ids = _prompt(4, 7)
    tok = _prompt(4, 8)[:, :1].contiguous()
    plain = GPTForGeneration(gpt, dict(static_kv_cache=True,
                                       kv_cache_dtype=kv, max_dec_len=2))
    want = _one_step(plain, deq32, ids, tok, prefill_model=gpt32)
    h_off = _one_step(gen_off, deq16, ids, tok, prefill_model=gpt)
    h_on = _one_step(gen_on, gpt, ids, tok)
    h_bf = _one_step(gen_off, gpt, ids, tok)
    e_off = float((h_off - want).abs().max())
    e_on = float((h_on - want).abs().max())
    d_q = float((h_on - h_bf).abs().max())
    print(f"\n[decode_linear_fp8] step {kv}: max-abs error vs fp32 "
          f"code*scale reference: fp8 path {e_on:.3e}, bf16 path on "
          f"dequantised weights {e_off:.3e}; distance of the fp8 step from "
          f"the unquantised bf16 step {d_q:.3e} (information)", end="")
    assert e_off > 0 and torch.isfinite(h_on).all()
    assert e_on <= 2 * e_off, (e_on, e_off)
