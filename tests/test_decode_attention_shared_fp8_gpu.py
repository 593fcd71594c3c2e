"""GPU: shared-prompt decode attention over an fp8 prompt prefix
(csrc/decode_attention_shared_fp8.hip) against a float64 reference, plus
StaticKVCache(shared_prefix_dtype="fp8") through the model and the captured
generation loop."""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import GPTModel, StaticKVCache
from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import decode_attention_shared, hip_ext
from paddlefleetx_amd.parallel.env import init_dist_env

LCAP, SCAP = 320, 8
SUF = (0, 1, 7)  # own tokens of row b: SUF[b % 3]
# (D, G, P, h, prefix length per prompt), the cases of the bf16 shared test
CASES = [(64, 2, 1, 1, (300,)), (128, 5, 3, 3, (0, 17, 300)),
         (128, 16, 1, 3, (33,)), (64, 17, 3, 1, (1, 15, 16)),
         (128, 17, 1, 1, (300,))]
SPLITS = [0, 1, 3, 7]
BF, F8 = torch.bfloat16, torch.float8_e4m3fn


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


@functools.lru_cache(maxsize=None)
def _case(ci, amp):
    """Inputs with NaN codes, scales and bf16 past every length, the float64
    reference over (code * scale) || own tokens || new token, and
    A = sum_j softmax_j |v_j|. Prefix row j is scaled by 2^(j % 7 - 3) before
    quantising (neighbours get different scales), row 0 of prompt 0 is zero.
    Built once per (case, amplitude); callers clone the caches."""
    D, G, P, h, plens = CASES[ci]
    B, dev = P * G, torch.device("cuda:0")
    g = torch.Generator().manual_seed(100 + ci)
    qkv = torch.randn(B, 1, h, 3, D, generator=g)
    kp, vp = torch.randn(2, P, h, LCAP, D, generator=g).unbind(0)
    kc, vc = torch.randn(2, B, h, SCAP, D, generator=g).unbind(0)
    qkv[:, :, :, :2] *= amp
    row = (2.0 ** (torch.arange(LCAP) % 7 - 3))[:, None]
    kp, vp, kc = kp * amp * row, vp * row, kc * amp
    kp[0, :, 0], vp[0, :, 0] = 0.0, 0.0
    qkv, kp, vp, kc, vc = (t.to(dev).to(BF).contiguous()
                           for t in (qkv, kp, vp, kc, vc))
    (kq, ks), (vq, vs) = ref.quantize_kv_rows(kp), ref.quantize_kv_rows(vp)
    assert (ks[0, :, 0] == 1).all() and (kq[0, :, 0].float() == 0).all()
    kd = kq.float().double() * ks.double()[..., None]
    vd = vq.float().double() * vs.double()[..., None]
    slens = [SUF[b % 3] for b in range(B)]
    want = torch.empty(B, h, D, dtype=torch.float64, device=dev)
    A = torch.empty_like(want)
    smax = 0.0
    for b in range(B):
        Lp, s = plens[b // G], slens[b]
        K = torch.cat((kd[b // G, :, :Lp], kc[b, :, :s].double(),
                       qkv[b, 0, :, 1:2].double()), 1)
        V = torch.cat((vd[b // G, :, :Lp], vc[b, :, :s].double(),
                       qkv[b, 0, :, 2:3].double()), 1)
        sc = torch.einsum("hd,hsd->hs", qkv[b, 0, :, 0].double(), K)
        smax = max(smax, sc.abs().max().item() / math.sqrt(D))
        p = torch.softmax(sc / math.sqrt(D), dim=-1)
        want[b] = torch.einsum("hs,hsd->hd", p, V)
        A[b] = torch.einsum("hs,hsd->hd", p, V.abs())
        kc[b, :, s:] = float("nan")
        vc[b, :, s:] = float("nan")
    for p_, Lp in enumerate(plens):
        kq.view(torch.uint8)[p_, :, Lp:] = 0x7F
        vq.view(torch.uint8)[p_, :, Lp:] = 0x7F
        ks[p_, :, Lp:] = float("nan")
        vs[p_, :, Lp:] = float("nan")
    pl = torch.tensor(plens, dtype=torch.int32, device=dev)
    total = torch.tensor([plens[b // G] + slens[b] for b in range(B)],
                         dtype=torch.int32, device=dev)
    return qkv, kq, vq, ks, vs, pl, kc, vc, total, slens, want, A, smax


def _run(c, kc, vc, G, splits, qkv=None):
    return decode_attention_shared(
        c[0] if qkv is None else qkv, c[1], c[2], c[5], kc, vc, c[8], G,
        max_prefix_len=LCAP, num_splits=splits, k_prefix_scale=c[3],
        v_prefix_scale=c[4])


@pytest.mark.parametrize(
    "ci,splits,amp",
    [(ci, s, 1.0) for ci in range(len(CASES)) for s in SPLITS]
    + [(ci, s, 5.5) for ci in (0, 1) for s in (1, 7)])
def test_numerics_containment_append(ci, splits, amp):
    """|y - r| <= 2^-8 |r| + 2^-7 A + 2^-126, the bound of the bf16 prefix:
    the bf16 roundings are y (2^-9) and p * v_scale before the second MFMA
    (2^-9 A); the decode is exact and the fp32 scale products sit orders
    below. Worst err/bound measured: 0.546."""
    D, G, P, h, plens = CASES[ci]
    c = _case(ci, amp)
    qkv, kc0, vc0, slens, want, A, smax = c[0], c[6], c[7], c[9], c[10], \
        c[11], c[12]
    assert amp == 1.0 or smax > 60.0
    fixed = [t.clone() for t in (c[1], c[2], c[3], c[4], c[5], c[8])]
    outs = []
    for _ in range(2):
        kc, vc = kc0.clone(), vc0.clone()
        outs.append(_run(c, kc, vc, G, splits))
    out = outs[0]
    assert out.shape == (P * G, 1, h * D) and out.dtype == BF
    assert torch.equal(out.view(torch.int16), outs[1].view(torch.int16))
    y = out.double().view(P * G, h, D)
    assert torch.isfinite(y).all()  # the NaN tails stayed out
    bound = 2.0 ** -8 * want.abs() + 2.0 ** -7 * A + 2.0 ** -126
    ratio = ((y - want).abs() / bound).max().item()
    print(f"case={CASES[ci]} splits={splits} amp={amp} err/bound={ratio:.3f}")
    assert ratio <= 1.0
    # append at the row's own length, bitwise; everything else unchanged
    for new, old, which in ((kc, kc0, 1), (vc, vc0, 2)):
        exp = old.clone().view(torch.int16)
        for b, s in enumerate(slens):
            exp[b, :, s] = qkv[b, 0, :, which].view(torch.int16)
        assert torch.equal(new.view(torch.int16), exp)
    for t, t0 in zip((c[1], c[2], c[3], c[4], c[5], c[8]), fixed):
        bits = torch.uint8 if t.dtype == F8 else torch.int32
        assert torch.equal(t.view(bits), t0.view(bits))
    for b, s in enumerate(slens):  # nothing cached: v_new bit for bit
        if s == 0 and plens[b // G] == 0:
            assert torch.equal(out[b, 0].view(torch.int16),
                               qkv[b, 0, :, 2].reshape(-1).view(torch.int16))


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("D", [64, 128])
def test_position_coverage_probe(D, splits):
    """K codes 0 give every valid position weight 1/(L+1); channel d of launch
    r carries a one-hot V (code 0x38 = 1.0, scale 1) at position r*D + d of
    prefix || own || new, so out[d]*(L+1) counts that position: 1 exactly.
    Past the lengths: NaN codes and NaN scales."""
    dev = torch.device("cuda:0")
    G, P, h, plens = 5, 3, 2, (300, 17, 0)
    B = P * G
    slens = [SUF[b % 3] for b in range(B)]
    pl = torch.tensor(plens, dtype=torch.int32, device=dev)
    total = torch.tensor([plens[b // G] + slens[b] for b in range(B)],
                         dtype=torch.int32, device=dev)
    for r in range((max(plens) + max(SUF) + 1 + D - 1) // D):
        pos = torch.arange(D, device=dev) + r * D
        ch = torch.arange(D, device=dev)
        qkv = torch.zeros(B, 1, h, 3, D, device=dev, dtype=BF)
        qkv[:, :, :, 0] = 0.5
        kq = torch.zeros(P, h, LCAP, D, device=dev, dtype=torch.uint8)
        vq = torch.zeros_like(kq)
        ks = torch.ones(P, h, LCAP, device=dev)
        vs = torch.ones_like(ks)
        kc = torch.zeros(B, h, SCAP, D, device=dev, dtype=BF)
        vc = torch.zeros_like(kc)
        expect = torch.zeros(B, h, D, device=dev)
        for p_, Lp in enumerate(plens):
            m = pos < Lp
            vq[p_, :, pos[m], ch[m]] = 0x38
            kq[p_, :, Lp:], vq[p_, :, Lp:] = 0x7F, 0x7F
            ks[p_, :, Lp:], vs[p_, :, Lp:] = float("nan"), float("nan")
        for b, s in enumerate(slens):
            Lp = plens[b // G]
            m = (pos >= Lp) & (pos < Lp + s)
            vc[b, :, pos[m] - Lp, ch[m]] = 1.0
            qkv[b, 0, :, 2, pos == Lp + s] = 1.0
            expect[b, :, pos <= Lp + s] = 1.0
            kc[b, :, s:], vc[b, :, s:] = float("nan"), float("nan")
        out = decode_attention_shared(
            qkv, kq.view(F8), vq.view(F8), pl, kc, vc, total, G,
            max_prefix_len=LCAP, num_splits=splits, k_prefix_scale=ks,
            v_prefix_scale=vs)
        counted = out.float().view(B, h, D) * (total + 1).float()[:, None, None]
        err = (counted - expect).abs().max().item()
        print(f"D={D} splits={splits} launch={r} max|count-expect|={err:.4f}")
        assert err <= 2e-2, (r, err)


def test_nan_query_stays_in_its_row():
    D, G, P, h, plens = CASES[3]  # G = 17: two column groups
    c = _case(3, 1.0)
    qkv = c[0].clone()
    bad = G + 1  # a sample of the second prompt
    qkv[bad, 0, :, 0] = float("nan")
    out = _run(c, c[6].clone(), c[7].clone(), G, 3, qkv=qkv)
    fin = torch.isfinite(out.float()).all(dim=-1).flatten()
    assert not fin[bad] and fin.sum() == P * G - 1


@pytest.mark.parametrize("change,match", [
    (dict(pdtype=BF), "float8_e4m3fn"), (dict(sdtype=torch.float16), "fp32"),
    (dict(slcap=15), "scales must be \\[P, h, Lcap\\]"),
    (dict(cdtype=F8), "k_cache and v_cache must be bf16"),
    (dict(group=0), "group"), (dict(mpl=17), "max_prefix_len"),
    # the checks shared with decode_attn_shared, through this entry point
    (dict(d=32), "head_dim"), (dict(P=2), "P \\* group"),
    (dict(group=4), "group"), (dict(mpl=0), "max_prefix_len"),
    (dict(splits=32), "num_splits"),
    (dict(lens_long=True), "seq_lens must be int32"),
    (dict(plens_long=True), "prefix_lens must be int32"),
    (dict(strided=True), "contiguous"), (dict(cpu=True), "on the GPU"),
    (dict(Scap_v=9), "v_cache shape"),
    (dict(qkv_offset=1), "16-byte aligned"),
])
def test_refusals(change, match):
    """Host checks fire before any launch and name the op."""
    dev = torch.device("cuda:0")
    c = dict(pdtype=F8, sdtype=torch.float32, slcap=16, cdtype=BF, group=2,
             mpl=16, d=64, P=3, splits=0, lens_long=False, plens_long=False,
             strided=False, cpu=False, Scap_v=8, qkv_offset=0)
    c.update(change)
    B, h, d, P = 6, 2, c["d"], c["P"]
    # a contiguous view qkv_offset bf16 elements into a larger buffer
    n = B * h * 3 * d
    qkv = torch.zeros(n + 8, device=dev, dtype=BF)[
        c["qkv_offset"]:c["qkv_offset"] + n].view(B, 1, h, 3, d)
    kp = torch.zeros(P, h, 16, d, device=dev).to(c["pdtype"])
    if c["strided"]:
        kp = kp.transpose(1, 2).contiguous().transpose(1, 2)
    sc = torch.ones(P, h, c["slcap"], device=dev, dtype=c["sdtype"])
    kc = torch.zeros(B, h, 8, d, device=dev).to(c["cdtype"])
    vc = torch.zeros(B, h, c["Scap_v"], d, device=dev).to(c["cdtype"])
    pl = torch.zeros(P, dtype=torch.int32, device=dev)
    lens = torch.zeros(B, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="decode_attn_shared_fp8.*" + match):
        hip_ext().decode_attn_shared_fp8(
            qkv, kp, kp.clone(), sc, sc.clone(),
            pl.long() if c["plens_long"] else pl, kc, vc,
            lens.long() if c["lens_long"] else lens.cpu() if c["cpu"]
            else lens, c["group"], 0.125, c["mpl"], c["splits"])


GPT = dict(vocab_size=512, hidden_size=256, num_layers=2,
           num_attention_heads=2, max_position_embeddings=64,
           hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def _gpu_gpt(dev):
    torch.manual_seed(11)
    with torch.device(dev):
        return GPTModel(dtype=BF, **GPT).eval()


def test_model_fp8_prefix_error_vs_fp32():
    """Teacher-forced prefill 16 + decode 6, P = 2, G = 3. e_new: the shared
    cache with an fp8 prefix; e_old: the unshared fp8 static cache, which
    quantises the same prompt rows and the generated ones too. The project's
    rule: e_new <= 2 e_old. Measured: e_old 0.01627, e_new 0.01441."""
    dev = torch.device("cuda:0")
    P, G, Lp, N = 2, 3, 16, 6
    B = P * G
    gpt = _gpu_gpt(dev)
    gpt32 = GPTModel(fused_attn=False, dtype=torch.float32, **GPT).eval()
    gpt32.load_state_dict({n: t.float().cpu()
                           for n, t in gpt.state_dict().items()})
    torch.manual_seed(5)
    ids = torch.cat((torch.randint(0, 512, (P, Lp)).repeat_interleave(G, 0),
                     torch.randint(0, 512, (B, N))), dim=1)
    pos = torch.arange(Lp + N).unsqueeze(0).expand(B, -1)
    with torch.no_grad():
        want = gpt32(ids, pos) @ gpt32.embeddings.word_embeddings.weight.t()
    ids, pos = ids.to(dev), pos.to(dev)
    gen = GPTForGeneration(gpt, {})
    old = StaticKVCache(2, B, 2, Lp + N, 128, dtype=BF, device=dev,
                        kv_dtype="fp8")
    new = StaticKVCache(2, B, 2, Lp + N, 128, dtype=BF, device=dev,
                        shared_group=G, suffix_len=N,
                        shared_prefix_dtype="fp8")
    with torch.no_grad():
        lo, _ = gen._logits(ids[:, :Lp], pos[:, :Lp], old)
        ln, _ = gen._logits(ids[::G, :Lp], pos[::G, :Lp], new)
        steps = [(Lp - 1, lo, ln.repeat_interleave(G, 0))]
        for t in range(Lp, Lp + N):
            lo, _ = gen._logits(ids[:, t:t + 1], pos[:, t:t + 1], old)
            ln, _ = gen._logits(ids[:, t:t + 1], pos[:, t:t + 1], new)
            steps.append((t, lo, ln))
    e_old = max((a.cpu() - want[:, t]).abs().max().item() for t, a, _ in steps)
    e_new = max((b.cpu() - want[:, t]).abs().max().item() for t, _, b in steps)
    print(f"e_old(unshared fp8)={e_old:.5f} e_new(fp8 prefix)={e_new:.5f}")
    assert new.max_len == Lp + N and e_old > 0.0
    assert e_new <= 2.0 * e_old, (e_new, e_old)


def test_captured_equals_eager():
    """shared_prompt_dtype: fp8: the captured loop gives the tokens, lens,
    prefix codes and scales and own K/V of the eager loop; ONE graph is
    replayed across prompt lengths."""
    dev = torch.device("cuda:0")
    gpt = _gpu_gpt(dev)
    cfg = {"max_dec_len": 8, "min_dec_len": 0, "eos_token_id": 511,
           "decoding_strategy": "sampling", "top_k": 8,
           "num_return_sequences": 3, "static_kv_cache": True,
           "fused_sampling": True, "shared_prompt_cache": True,
           "shared_prompt_dtype": "fp8", "kv_cache_capacity": 32}
    eager = GPTForGeneration(gpt, dict(cfg))
    capt = GPTForGeneration(gpt, dict(cfg, capture_decode=True))
    graphs = set()
    with torch.no_grad():
        for seed, plen in ((3, 5), (4, 7), (3, 5)):
            torch.manual_seed(seed)
            ids = torch.randint(0, 511, (2, plen), device=dev)
            torch.manual_seed(seed)
            oe, se = eager._sample_fused(ids, return_state=True)
            torch.manual_seed(seed)
            oc, sc = capt._sample_fused(ids, return_state=True)
            assert oe.shape[0] == 6 and torch.equal(oe, oc)
            own = oe.shape[1] - 1  # decode steps both loops surely ran
            ce, cc = se["cache"], sc["cache"]
            assert ce.k_prefix[0].dtype == F8
            assert torch.equal(ce.lens, cc.lens)
            assert torch.equal(ce.prefix_lens, cc.prefix_lens)
            for name, n in (("k", own), ("v", own), ("k_prefix", plen),
                            ("v_prefix", plen), ("k_prefix_scale", plen),
                            ("v_prefix_scale", plen)):
                for a, b in zip(getattr(ce, name), getattr(cc, name)):
                    a, b = a[:, :, :n].contiguous(), b[:, :, :n].contiguous()
                    assert torch.equal(a.view(torch.uint8),
                                       b.view(torch.uint8)), name
            graphs.add(sc["graph"])
    assert len(graphs) == 1
