"""GPU: the decode_linear kernel against float64, its masking, isolation,
determinism and refusals, and the fused decode layer on a tiny GPT.

Accuracy bound (derived, not tuned), r = act(x W^T + b) + res in float64
from the same bf16 inputs, S = |x| |W|^T + |b| + |res|:

    |y - r| <= 2^-8 |r| + 2 K 2^-24 S + 2^-126

2^-8 |r| is the one rounding to bf16, 2 K 2^-24 S the fp32 accumulation of K
exact bf16 products (factor 2 for the MFMA's internal order). With gelu the
project's fp32 bias-gelu tolerance (FP32_TOL["bg.y"] of
test_ops_edges_gpu.py) is added for the hardware-exp tanh.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_ops_edges_gpu import FP32_TOL

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import GPTModel
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_linear, hip_ext
from paddlefleetx_amd.parallel.env import init_dist_env

DEV = "cuda:0"
BF16, F64 = torch.bfloat16, torch.float64

SHAPES = [(16, 32), (24, 96), (384, 128), (128, 512), (512, 128),
          (2048, 2080), (50304, 128)]
MS = [1, 2, 5, 16]
CASES = [(n, k, m) for (n, k) in SHAPES for m in MS] + [(2048, 8192, 16)]
# (bias, activation, residual)
EPILOGUES = {"none": (False, None, False), "bias": (True, None, False),
             "bias_gelu": (True, "gelu", False),
             "bias_res": (True, None, True), "res": (False, None, True)}

_INPUTS = {}
_REFS = {}


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


def _inputs(N, K):
    """16 rows of x, W, bias and residual for one (N, K); smaller M are
    leading-row slices, so every case of a shape shares one set."""
    if (N, K) not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * N + K)
        x = torch.randn(16, K, generator=g).to(BF16).to(DEV)
        w = (torch.randn(N, K, generator=g) * 0.05).to(BF16).to(DEV)
        b = torch.randn(N, generator=g).to(BF16).to(DEV)
        r = torch.randn(16, N, generator=g).to(BF16).to(DEV)
        _INPUTS[(N, K)] = (x, w, b, r)
    return _INPUTS[(N, K)]


def _gelu64(y):
    return 0.5 * y * (1.0 + torch.tanh(
        0.7978845608028654 * (y + 0.044715 * y ** 3)))


def _reference(N, K, ep):
    """float64 (r, S) for all 16 rows of one shape and epilogue, computed
    once and never modified."""
    key = (N, K, ep)
    if key not in _REFS:
        x, w, b, r = _inputs(N, K)
        bias, act, res = EPILOGUES[ep]
        y = x.to(F64) @ w.to(F64).t()
        s = x.to(F64).abs() @ w.to(F64).abs().t()
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
    bound = 2.0 ** -8 * want.abs() + 2 * K * 2.0 ** -24 * s + 2.0 ** -126
    if gelu:
        rtol, atol = FP32_TOL["bg.y"]
        bound = bound + atol + rtol * want.abs()
    return bound


def _check(got, want, s, K, gelu, what):
    assert got.dtype == BF16 and got.shape == want.shape, what
    err = (got.to(F64) - want).abs()
    bound = _bound(want, s, K, gelu)
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max())
    print(f"\n[decode_linear] {what}: worst err/bound = {ratio:.3g}", end="")
    assert ratio <= 1.0, f"{what}: {ratio:.3g} x bound"


def _args(N, K, M, ep):
    x, w, b, r = _inputs(N, K)
    bias, act, res = EPILOGUES[ep]
    return (x[:M], w, b if bias else None, r[:M] if res else None, act)


@pytest.mark.parametrize("ep", list(EPILOGUES))
@pytest.mark.parametrize("N,K,M", CASES)
def test_accuracy_against_float64(N, K, M, ep):
    args = _args(N, K, M, ep)
    got = decode_linear(*args)
    want, s = _reference(N, K, ep)
    _check(got, want[:M], s[:M], K, args[4] == "gelu", f"{N}x{K} M={M} {ep}")
    # the op took the kernel: same bits as the binding called directly
    direct = hip_ext().decode_linear(args[0], args[1], args[2], args[3],
                                     args[4] or "none")
    assert torch.equal(got, direct)


@pytest.mark.parametrize("rows,waves,nt",
                         [(rows, waves, nt) for rows in (8, 16, 32)
                          for waves in (4, 8) for nt in (0, 1)])
@pytest.mark.parametrize("N,K,M", [(24, 96, 5), (2048, 2080, 16)])
def test_every_kernel_variant_is_accurate(N, K, M, rows, waves, nt):
    """The automatic choice reaches only some (rows, waves, nt) instances on
    the shapes above; the overrides reach the others."""
    x, w, b, r = _args(N, K, M, "bias_res")[:4]
    got = hip_ext().decode_linear(x, w, b, r, "none", rows, waves, nt)
    want, s = _reference(N, K, "bias_res")
    _check(got, want[:M], s[:M], K, False,
           f"{N}x{K} M={M} rows={rows} waves={waves} nt={nt}")


@pytest.mark.parametrize("ep", ["bias_gelu", "bias_res"])
@pytest.mark.parametrize("M", MS)
def test_rows_past_m_and_n_are_never_read(M, ep):
    N, K = 24, 96
    x, w, b, r = _inputs(N, K)
    xbuf = torch.full((32, K), float("nan"), dtype=BF16, device=DEV)
    wbuf = torch.full((N + 40, K), float("nan"), dtype=BF16, device=DEV)
    xbuf[:M] = x[:M]
    wbuf[:N] = w
    bias, act, res = EPILOGUES[ep]
    got = decode_linear(xbuf[:M], wbuf[:N], b, r[:M] if res else None, act)
    assert bool(torch.isfinite(got).all())
    want, s = _reference(N, K, ep)
    _check(got, want[:M], s[:M], K, act == "gelu", f"masked M={M} {ep}")
    assert torch.equal(got, decode_linear(*_args(N, K, M, ep)))


@pytest.mark.parametrize("N,K", [(24, 96), (2048, 2080)])
@pytest.mark.parametrize("M", [2, 5, 16])
def test_rows_are_isolated(N, K, M):
    x, w, b, r = _args(N, K, M, "bias_res")[:4]
    clean = decode_linear(x, w, b, r)
    bad = x.clone()
    bad[0, K // 2 + 3] = float("inf")
    got = decode_linear(bad, w, b, r)
    assert torch.equal(got[1:], clean[1:])
    assert not bool(torch.isfinite(got[0]).any())


@pytest.mark.parametrize("N,K,M", [(24, 96, 5), (2048, 2080, 16),
                                   (50304, 128, 2)])
def test_two_calls_are_bitwise_equal(N, K, M):
    args = _args(N, K, M, "bias_gelu")
    a = decode_linear(*args)
    b = decode_linear(*args)
    assert torch.equal(a, b)


def _refused(x, w):
    """(kwargs that make the binding raise, what the op still accepts)."""
    ext = hip_ext()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="decode_linear"):
        ext.decode_linear(x, w)
    torch.cuda.synchronize()  # and nothing was left in flight to fail later
    got = decode_linear(x, w)
    want = ref.decode_linear(x, w)
    assert got.shape == want.shape and got.dtype == want.dtype
    s = x.to(F64).abs() @ w.to(F64).abs().t()
    K = x.shape[1]
    # library GEMM against the fp32 twin: each rounds once to the dtype and
    # sums K products in fp32 in its own order
    eps = 2.0 ** -8 if x.dtype == BF16 else 2.0 ** -24
    bound = eps * s + 2 * K * 2.0 ** -23 * s + 2.0 ** -126
    err = (got.to(F64) - want.to(F64)).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


def test_binding_refuses_and_op_falls_back():
    g = torch.Generator().manual_seed(3)

    def rnd(*shape, dtype=BF16):
        return (torch.randn(*shape, generator=g) * 0.1).to(dtype).to(DEV)

    _refused(rnd(17, 64), rnd(24, 64))                       # M = 17
    _refused(rnd(4, 40), rnd(24, 40))                        # K = 40
    _refused(rnd(4, 64, dtype=torch.float32),
             rnd(24, 64, dtype=torch.float32))               # fp32 x
    _refused(rnd(4, 64), rnd(24, 128)[:, ::2])               # strided weight
    ext = hip_ext()
    x, w = rnd(4, 64), rnd(24, 64)
    for bad in (dict(bias=rnd(16)), dict(residual=rnd(4, 16)),
                dict(act="relu"), dict(bias=rnd(24).float()),
                dict(rows=4), dict(waves=2), dict(nontemporal=2), dict(weight=rnd(20, 64))):
        kw = dict(x=x, weight=w)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="decode_linear"):
            ext.decode_linear(**kw)
    with pytest.raises(RuntimeError, match="decode_linear"):
        ext.decode_linear(x.cpu(), w.cpu())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# model level: the tiny GPT of test_decode_graph_gpu.py
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
                fused_decode_linear=True, **kw)


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
def test_captured_equals_eager_with_fused_linear(gpt, kv, monkeypatch):
    calls = []
    ext = hip_ext()
    from paddlefleetx_amd.ops import functional
    real = functional.hip_ext

    class Counting:
        def __getattr__(self, name):
            if name == "decode_linear":
                calls.append(1)
            return getattr(ext, name)

    monkeypatch.setattr(functional, "hip_ext", lambda: Counting())
    eager = GPTForGeneration(gpt, _cfg(kv))
    captured = GPTForGeneration(gpt, _cfg(kv, capture_decode=True))
    ids = _prompt(2, 3)
    e1 = _generate(eager, ids, 21)
    # the kernel itself ran: 4 per layer + the logits, every decode step
    assert len(calls) == (NEW - 1) * (4 * len(gpt.layers) + 1)
    monkeypatch.setattr(functional, "hip_ext", real)
    c1 = _generate(captured, ids, 21)
    _assert_same(c1, e1)
    # a second prompt replays the same graph
    graph = captured._graph_state["graph"]
    ids2 = _prompt(2, 4)
    _assert_same(_generate(captured, ids2, 22), _generate(eager, ids2, 22))
    assert captured._graph_state["graph"] is graph


def _one_step(gen, model, ids, tok):
    B, P = ids.shape
    cache = gen._new_static_cache(B, P + 2, ids.device)
    if model.embeddings.word_embeddings.weight.dtype != torch.bfloat16:
        # the fp32 reference model keeps an fp32 cache
        from paddlefleetx_amd.models.gpt.model import StaticKVCache
        attn = model.layers[0].attn
        cache = StaticKVCache(len(model.layers), B, attn.num_heads_local,
                              P + 2, attn.head_dim, dtype=torch.float32,
                              device=ids.device)
    pos = torch.arange(P, device=ids.device).unsqueeze(0).expand(B, -1)
    with torch.no_grad():
        model(ids, pos, caches=cache, use_cache=True)
        hidden, _ = model(tok, cache.lens.long().unsqueeze(1), caches=cache,
                          use_cache=True)
    return hidden.float()


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_teacher_forced_step_is_no_worse_than_existing_path(gpt, kv):
    import copy
    cfg = dict(static_kv_cache=True, kv_cache_dtype=kv, max_dec_len=2)
    gen_off = GPTForGeneration(gpt, cfg)
    gen_on = GPTForGeneration(gpt, dict(cfg, fused_decode_linear=True))
    gpt32 = copy.deepcopy(gpt).float()
    for layer in gpt32.layers:
        layer.attn.fused_attn = False  # the flash kernel is bf16 only
    ids = _prompt(4, 7)
    tok = _prompt(4, 8)[:, :1].contiguous()
    want = _one_step(gen_off, gpt32, ids, tok)
    h_off = _one_step(gen_off, gpt, ids, tok)
    h_on = _one_step(gen_on, gpt, ids, tok)
    e_off = float((h_off - want).abs().max())
    e_on = float((h_on - want).abs().max())
    print(f"\n[decode_linear] step {kv}: max-abs error vs fp32 reference "
          f"flag on {e_on:.3e}, flag off {e_off:.3e}", end="")
    assert e_off > 0 and torch.isfinite(h_on).all()
    assert e_on <= 2 * e_off, (e_on, e_off)
