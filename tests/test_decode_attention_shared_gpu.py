"""GPU: shared-prompt decode attention (csrc/decode_attention_shared.hip)
against a float64 reference, plus the shared-prompt StaticKVCache through the
model and the captured generation loop."""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from paddlefleetx_amd.models.gpt.generation import GPTForGeneration
from paddlefleetx_amd.models.gpt.model import GPTModel, StaticKVCache
from paddlefleetx_amd.ops import decode_attention_shared, hip_ext
from paddlefleetx_amd.parallel.env import init_dist_env

LCAP, SCAP = 320, 8
SUF = (0, 1, 7)  # own tokens of row b: SUF[b % 3], different within a group
# (D, G, P, h, prefix length per prompt): every D, G, P, h and prefix length
# of the plan; G = 17 is two column groups, the second with one live column;
# 15/16/17/33 sit on the 16- and 32-position tile edges, 300 spans chunks
CASES = [(64, 2, 1, 1, (300,)), (128, 5, 3, 3, (0, 17, 300)),
         (128, 16, 1, 3, (33,)), (64, 17, 3, 1, (1, 15, 16)),
         (128, 17, 1, 1, (300,))]
SPLITS = [0, 1, 3, 7]  # 7: short prefixes own empty chunks
BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _env():
    init_dist_env({"Distributed": {}})


@functools.lru_cache(maxsize=None)
def _case(ci, amp):
    """bf16 inputs with NaN past every length, the float64 reference over
    prefix || own tokens || new token, and A = sum_j softmax_j |v_j|; built
    once per (case, amplitude) and shared; callers clone the caches."""
    D, G, P, h, plens = CASES[ci]
    B, dev = P * G, torch.device("cuda:0")
    g = torch.Generator().manual_seed(100 + ci)
    qkv = torch.randn(B, 1, h, 3, D, generator=g)
    kp, vp = torch.randn(2, P, h, LCAP, D, generator=g).unbind(0)
    kc, vc = torch.randn(2, B, h, SCAP, D, generator=g).unbind(0)
    qkv[:, :, :, :2] *= amp
    kp, kc = kp * amp, kc * amp
    qkv, kp, vp, kc, vc = (t.to(dev).to(BF).contiguous()
                           for t in (qkv, kp, vp, kc, vc))
    slens = [SUF[b % 3] for b in range(B)]
    want = torch.empty(B, h, D, dtype=torch.float64, device=dev)
    A = torch.empty_like(want)
    smax = 0.0
    for b in range(B):
        Lp, s = plens[b // G], slens[b]
        K = torch.cat((kp[b // G, :, :Lp], kc[b, :, :s], qkv[b, 0, :, 1:2]), 1)
        V = torch.cat((vp[b // G, :, :Lp], vc[b, :, :s], qkv[b, 0, :, 2:3]), 1)
        sc = torch.einsum("hd,hsd->hs", qkv[b, 0, :, 0].double(), K.double())
        smax = max(smax, sc.abs().max().item() / math.sqrt(D))
        p = torch.softmax(sc / math.sqrt(D), dim=-1)
        want[b] = torch.einsum("hs,hsd->hd", p, V.double())
        A[b] = torch.einsum("hs,hsd->hd", p, V.double().abs())
        kc[b, :, s:] = float("nan")
        vc[b, :, s:] = float("nan")
    for p_, Lp in enumerate(plens):
        kp[p_, :, Lp:] = float("nan")
        vp[p_, :, Lp:] = float("nan")
    pl = torch.tensor(plens, dtype=torch.int32, device=dev)
    total = torch.tensor([plens[b // G] + slens[b] for b in range(B)],
                         dtype=torch.int32, device=dev)
    return qkv, kp, vp, pl, kc, vc, total, slens, want, A, smax


# amplitude 5.5 (|score| > 60: the online rescale and the merge) on the two
# long-prefix cases, one chunk and seven
@pytest.mark.parametrize(
    "ci,splits,amp",
    [(ci, s, 1.0) for ci in range(len(CASES)) for s in SPLITS]
    + [(ci, s, 5.5) for ci in (0, 1) for s in (1, 7)])
def test_numerics_containment_append(ci, splits, amp):
    """|y - r| <= 2^-8 |r| + 2^-7 A + 2^-126: one bf16 rounding of y (2^-9),
    one of each p before the second MFMA (2^-9 A), fp32 errors orders below,
    a factor 2 to 4 of slack each."""
    D, G, P, h, plens = CASES[ci]
    qkv, kp, vp, pl, kc0, vc0, total, slens, want, A, smax = _case(ci, amp)
    assert amp == 1.0 or smax > 60.0
    kp0, vp0, pl0, total0 = kp.clone(), vp.clone(), pl.clone(), total.clone()
    outs = []
    for _ in range(2):
        kc, vc = kc0.clone(), vc0.clone()
        outs.append(decode_attention_shared(
            qkv, kp, vp, pl, kc, vc, total, G, max_prefix_len=LCAP,
            num_splits=splits))
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
    for t, t0 in ((kp, kp0), (vp, vp0), (pl, pl0), (total, total0)):
        assert torch.equal(t.view(torch.int16), t0.view(torch.int16))
    for b, s in enumerate(slens):  # nothing cached: v_new bit for bit
        if s == 0 and plens[b // G] == 0:
            assert torch.equal(out[b, 0].view(torch.int16),
                               qkv[b, 0, :, 2].reshape(-1).view(torch.int16))


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("D", [64, 128])
def test_position_coverage_probe(D, splits):
    """K = 0 gives every valid position weight 1/(L+1); channel d of launch
    r carries a one-hot V at position r*D + d of prefix || own || new, so
    out[d]*(L+1) counts that position: 1 exactly. Past the lengths: 1000."""
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
        kp = torch.zeros(P, h, LCAP, D, device=dev, dtype=BF)
        vp, kc = torch.zeros_like(kp), torch.zeros(B, h, SCAP, D, device=dev,
                                                   dtype=BF)
        vc = torch.zeros_like(kc)
        expect = torch.zeros(B, h, D, device=dev)
        for p_, Lp in enumerate(plens):
            m = pos < Lp
            vp[p_, :, pos[m], ch[m]] = 1.0
            kp[p_, :, Lp:] = 1000.0
            vp[p_, :, Lp:] = 1000.0
        for b, s in enumerate(slens):
            Lp = plens[b // G]
            m = (pos >= Lp) & (pos < Lp + s)
            vc[b, :, pos[m] - Lp, ch[m]] = 1.0
            qkv[b, 0, :, 2, pos == Lp + s] = 1.0
            expect[b, :, pos <= Lp + s] = 1.0
            kc[b, :, s:] = 1000.0
            vc[b, :, s:] = 1000.0
        out = decode_attention_shared(qkv, kp, vp, pl, kc, vc, total, G,
                                      max_prefix_len=LCAP, num_splits=splits)
        counted = out.float().view(B, h, D) * (total + 1).float()[:, None, None]
        err = (counted - expect).abs().max().item()
        print(f"D={D} splits={splits} launch={r} max|count-expect|={err:.4f}")
        assert err <= 2e-2, (r, err)


@pytest.mark.parametrize("ci", [1, 3])
def test_nan_query_stays_in_its_row(ci):
    D, G, P, h, plens = CASES[ci]
    qkv, kp, vp, pl, kc, vc, total = _case(ci, 1.0)[:7]
    qkv = qkv.clone()
    bad = G + 1  # a sample of the second prompt
    qkv[bad, 0, :, 0] = float("nan")
    out = decode_attention_shared(qkv, kp, vp, pl, kc.clone(), vc.clone(),
                                  total, G, max_prefix_len=LCAP, num_splits=3)
    fin = torch.isfinite(out.float()).all(dim=-1).flatten()
    assert not fin[bad] and fin.sum() == P * G - 1


@pytest.mark.parametrize("change,match", [
    (dict(dtype=torch.float16), "bf16"), (dict(d=32), "head_dim"),
    (dict(group=0), "group"), (dict(group=4), "group"),
    (dict(P=2), "P \\* group"), (dict(mpl=0), "max_prefix_len"),
    (dict(mpl=17), "max_prefix_len"), (dict(splits=32), "num_splits"),
    (dict(lens_long=True), "seq_lens must be int32"),
    (dict(plens_long=True), "prefix_lens must be int32"),
    (dict(strided=True), "contiguous"), (dict(cpu=True), "on the GPU"),
    (dict(Scap_v=9), "v_cache shape"),
])
def test_refusals(change, match):
    """Host checks fire before any launch and name the op."""
    dev = torch.device("cuda:0")
    c = dict(dtype=BF, d=64, group=2, P=3, mpl=16, splits=0, lens_long=False,
             plens_long=False, strided=False, cpu=False, Scap_v=8)
    c.update(change)
    B, h, d = 6, 2, c["d"]
    qkv = torch.zeros(B, 1, h, 3, d, device=dev, dtype=c["dtype"])
    kp = torch.zeros(c["P"], h, 16, d, device=dev, dtype=c["dtype"])
    vp = torch.zeros_like(kp)
    kc = torch.zeros(B, h, 8, d, device=dev, dtype=c["dtype"])
    vc = torch.zeros(B, h, c["Scap_v"], d, device=dev, dtype=c["dtype"])
    pl = torch.zeros(c["P"], dtype=torch.int32, device=dev)
    lens = torch.zeros(B, dtype=torch.int32, device=dev)
    if c["strided"]:
        kp = kp.transpose(1, 2).contiguous().transpose(1, 2)
    with pytest.raises(RuntimeError, match="decode_attn_shared.*" + match):
        hip_ext().decode_attn_shared(
            qkv, kp, vp, pl.long() if c["plens_long"] else pl, kc, vc,
            lens.long() if c["lens_long"] else lens.cpu() if c["cpu"]
            else lens, c["group"], 0.125, c["mpl"], c["splits"])


def _gpu_gpt(dev, dtype):
    torch.manual_seed(11)
    with torch.device(dev):
        return GPTModel(vocab_size=512, hidden_size=256, num_layers=2,
                        num_attention_heads=2, max_position_embeddings=64,
                        hidden_dropout_prob=0.0,
                        attention_probs_dropout_prob=0.0, dtype=dtype).eval()


def test_model_shared_cache_error_vs_fp32():
    """Teacher-forced prefill 16 + decode 6, P = 2, G = 3. Shared and
    unshared static-cache logits are both bf16 roundings of the fp32 model's;
    the shared path may be at most 2x as far from fp32 as the unshared one
    (the rule of test_model_static_cache_error_vs_fp32)."""
    dev = torch.device("cuda:0")
    P, G, Lp, N = 2, 3, 16, 6
    B = P * G
    gpt = _gpu_gpt(dev, BF)
    gpt32 = GPTModel(vocab_size=512, hidden_size=256, num_layers=2,
                     num_attention_heads=2, max_position_embeddings=64,
                     hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0, fused_attn=False,
                     dtype=torch.float32).eval()
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
    plain = StaticKVCache(2, B, 2, Lp + N, 128, dtype=BF, device=dev)
    shared = StaticKVCache(2, B, 2, Lp + N, 128, dtype=BF, device=dev,
                           shared_group=G, suffix_len=N)
    with torch.no_grad():
        lu, _ = gen._logits(ids[:, :Lp], pos[:, :Lp], plain)
        ls, _ = gen._logits(ids[::G, :Lp], pos[::G, :Lp], shared)
        steps = [(Lp - 1, lu, ls.repeat_interleave(G, 0))]
        for t in range(Lp, Lp + N):
            lu, _ = gen._logits(ids[:, t:t + 1], pos[:, t:t + 1], plain)
            ls, _ = gen._logits(ids[:, t:t + 1], pos[:, t:t + 1], shared)
            steps.append((t, lu, ls))
    e_u = max((lu.cpu() - want[:, t]).abs().max().item() for t, lu, _ in steps)
    e_s = max((ls.cpu() - want[:, t]).abs().max().item() for t, _, ls in steps)
    print(f"e_unshared={e_u:.5f} e_shared={e_s:.5f}")
    assert shared.max_len == Lp + N and e_u > 0.0
    assert e_s <= 2.0 * e_u, (e_s, e_u)


def test_captured_equals_eager():
    """Flag on: the captured loop gives the tokens, lens and cached K/V of
    the eager loop at the same kv_cache_capacity; min_dec_len 0 keeps the
    graph key fixed, so ONE graph is replayed across prompt lengths."""
    dev = torch.device("cuda:0")
    gpt = _gpu_gpt(dev, BF)
    cfg = {"max_dec_len": 8, "min_dec_len": 0, "eos_token_id": 511,
           "decoding_strategy": "sampling", "top_k": 8,
           "num_return_sequences": 3, "static_kv_cache": True,
           "fused_sampling": True, "shared_prompt_cache": True,
           "kv_cache_capacity": 32}
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
            assert torch.equal(ce.lens, cc.lens)
            assert torch.equal(ce.prefix_lens, cc.prefix_lens)
            for i in range(2):
                for a, b in ((ce.k[i], cc.k[i]), (ce.v[i], cc.v[i])):
                    assert torch.equal(a[:, :, :own].view(torch.int16),
                                       b[:, :, :own].view(torch.int16))
                for a, b in ((ce.k_prefix[i], cc.k_prefix[i]),
                             (ce.v_prefix[i], cc.v_prefix[i])):
                    assert torch.equal(a[:, :, :plen].view(torch.int16),
                                       b[:, :, :plen].view(torch.int16))
            graphs.add(sc["graph"])
    assert len(graphs) == 1
