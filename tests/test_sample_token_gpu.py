"""GPU: the fused sampler kernel (csrc/sample_token.hip) against its fp32 twin
(exactly, at small V, on inputs with asserted fp64 margins) and against fp64
bands at the full vocabulary."""

import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from paddlefleetx_amd.ops import _reference as ref
from paddlefleetx_amd.ops import hip_ext, sample_token

T = 12
MIN_LENGTH = 7
LENS = [5, 9, 3, 11, 7, 6, 8, 10, 4, 9, 5, 11, 6, 8, 3, 12]  # row 15 is full
MARGIN = 4e-4  # nucleus mass clears top_p by this much, both sides (fp64)
GAP = 1e-5     # relative gap of two probabilities that must not tie in fp32
TOP_KS = lambda V: [0, 1, 8, V]
TOP_PS = [1.0, 0.9, 0.5, 1e-6]
PENS = [1.0, 1.3]
TEMPS = [1.0, 0.7]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    hip_ext()
    return torch.device("cuda:0")


# -- fp64 oracle ------------------------------------------------------------------

def _oracle(z, top_k, top_p):
    """z: processed logits / temperature, fp32-exact values as float64 [V].
    Tie-inclusive top-k then top-p in fp64. Returns p, keep and the two
    masses that bracket top_p: ahead of the last kept tie group, and of the
    whole kept set (None where top-p drops nothing)."""
    V = z.numel()
    p = torch.softmax(z, dim=-1)
    q = p
    gaps = []
    if 0 < top_k < V:
        s = torch.sort(p, descending=True).values
        gaps.append((s[top_k - 1], s[top_k]))
        q = torch.where(p >= s[top_k - 1], p, torch.zeros_like(p))
    ahead_last = kept_mass = None
    if top_p < 1.0:
        s = torch.sort(q, descending=True).values
        c = torch.cumsum(s, 0)
        # mass strictly greater than each sorted value (ties share it)
        first = torch.searchsorted(-s, -s, right=False)  # first index of tie group
        ahead = torch.where(first > 0, c[(first - 1).clamp(min=0)],
                            torch.zeros_like(c))
        kept_sorted = (ahead <= top_p) & (s > 0)
        n = int(kept_sorted.sum())
        last = s[n - 1]
        ahead_last = float(ahead[n - 1])
        if n < V and s[n] > 0:
            kept_mass = float(ahead[n])
            gaps.append((s[n - 1], s[n]))
        else:
            kept_mass_all = float(c[n - 1])
            kept_mass = None if kept_mass_all > top_p else kept_mass_all
        q = torch.where(q >= last, q, torch.zeros_like(q))
    gap_ok = all(a == b or float((a - b) / a) > GAP for a, b in gaps)
    return p, q > 0, ahead_last, kept_mass, gap_ok


def _nucleus_margin_ok(top_p, ahead_last, kept_mass):
    if top_p not in (0.9, 0.5):
        return True
    if ahead_last > 0 and ahead_last > top_p - MARGIN:
        return False
    if kept_mass is None:
        return True
    # kept set either exceeds top_p (something was dropped) or is everything
    return abs(kept_mass - top_p) >= MARGIN


def _draw_margin_ok(p, keep, u, delta):
    kept = torch.where(keep, p, torch.zeros_like(p))
    cum = torch.cumsum(kept, 0)
    mass = cum[-1]
    return float((cum - u * mass).abs().min()) >= delta * float(mass)


# -- inputs -----------------------------------------------------------------------

def _row_logits(V, b, seed, dtype, eos):
    g = torch.Generator().manual_seed(seed)
    row = 3.0 * torch.randn(V, generator=g)
    row[(7 * b + 3) % V] = -float("inf")
    if b % 2:
        row[0] = -float("inf")
    if b == 1:
        row[eos] = 25.0  # this row draws eos (no underflow at T = 0.7)
    return row.to(dtype)


def _history(V, b):
    g = torch.Generator().manual_seed(900 + b)
    h = torch.randint(0, V, (T,), generator=g)
    h[1] = h[0]  # duplicated history token
    return h


def _row_ok(V, b, row, hist, u, eos):
    """All fp64 margins of the small-V comparison, for every parameter
    combination."""
    lens = torch.tensor([LENS[b]], dtype=torch.int32)
    delta = V * 2.0 ** -23
    for pen, temp in itertools.product(PENS, TEMPS):
        x, _, _ = ref.sample_token_filter(row[None], hist[None], lens, 1.0, 0,
                                          1.0, pen, MIN_LENGTH, eos)
        z = (x[0] / temp if temp != 1.0 else x[0]).double()
        for top_k, top_p in itertools.product(TOP_KS(V), TOP_PS):
            p, keep, ahead_last, kept_mass, gap_ok = _oracle(z, top_k, top_p)
            if not (gap_ok and _nucleus_margin_ok(top_p, ahead_last, kept_mass)
                    and _draw_margin_ok(p, keep, float(u), delta)):
                return False
    return True


@functools.lru_cache(maxsize=None)
def _small_inputs(V, dtype):
    """16 rows of 3 * randn logits, each from the first seed (counting up from
    1000 * row) whose fp64 margins hold; callers use the first B rows."""
    eos = V - 2
    g = torch.Generator().manual_seed(77)
    u = torch.rand(16, T, generator=g)
    rows, hists, seeds = [], [], []
    for b in range(16):
        hist = _history(V, b)
        ub = u[b, min(LENS[b], T - 1)]
        for seed in range(1000 * b, 1000 * b + 200):
            row = _row_logits(V, b, seed, dtype, eos)
            if _row_ok(V, b, row, hist, ub, eos):
                break
        else:
            raise AssertionError(f"no seed with margins for row {b}")
        rows.append(row), hists.append(hist), seeds.append(seed)
    return torch.stack(rows), torch.stack(hists), u, eos


def _state(B, hists, u, device):
    unfinished = torch.ones(B, dtype=torch.bool)
    if B >= 3:
        unfinished[2] = False  # a row already finished
    return dict(ids_buf=hists[:B].clone().to(device),
                lens=torch.tensor(LENS[:B], dtype=torch.int32, device=device),
                unfinished=unfinished.to(device),
                u=u[:B].clone().to(device),
                next_tokens=torch.full((B, 1), -7, dtype=torch.long,
                                       device=device))


def _run(logits, st, **kw):
    count, mass = sample_token(logits, st["ids_buf"], st["lens"],
                               st["unfinished"], st["u"], st["next_tokens"],
                               **kw)
    return count, mass


# -- small V: exact against the twin ---------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("V", [257, 1000])
def test_small_vocab_equals_twin(dev, V, B, dtype):
    rows, hists, u, eos = _small_inputs(V, dtype)
    logits = rows[:B]
    # the margins that make an exact comparison fair, asserted from fp64
    for b in range(B):
        assert _row_ok(V, b, logits[b], hists[b], u[b, min(LENS[b], T - 1)],
                       eos)
    dlogits = logits.to(dev)
    checked = 0
    for top_k, top_p, pen, temp in itertools.product(TOP_KS(V), TOP_PS, PENS,
                                                     TEMPS):
        kw = dict(temperature=temp, top_k=top_k, top_p=top_p,
                  repetition_penalty=pen, min_length=MIN_LENGTH,
                  eos_token_id=eos, pad_token_id=1)
        want, got = _state(B, hists, u, "cpu"), _state(B, hists, u, dev)
        wc, wm = _run(logits, want, **kw)
        gc, gm = _run(dlogits, got, **kw)
        tag = (top_k, top_p, pen, temp)
        assert torch.equal(gc.cpu(), wc), tag
        assert torch.equal(got["next_tokens"].cpu(), want["next_tokens"]), tag
        assert torch.equal(got["ids_buf"].cpu(), want["ids_buf"]), tag
        assert torch.equal(got["unfinished"].cpu(), want["unfinished"]), tag
        torch.testing.assert_close(gm.cpu(), wm, rtol=V * 2.0 ** -23, atol=0)
        assert (wc >= 1).all(), tag
        if B >= 3:
            assert want["next_tokens"][1, 0] == eos  # the row that draws eos
            assert not want["unfinished"][1]
            assert want["next_tokens"][2, 0] == 1    # finished row: pad
            # min_length on both sides of lens within the batch
            assert LENS[0] < MIN_LENGTH <= LENS[1]
        checked += 1
    assert checked == 64


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [257, 1000])
def test_small_vocab_greedy_and_min_length(dev, V, dtype):
    rows, hists, u, eos = _small_inputs(V, dtype)
    B = 16
    logits = rows.clone()
    logits[:, eos] = 50.0  # eos is the arg-max wherever it is allowed
    for pen in PENS:
        kw = dict(greedy=True, repetition_penalty=pen, min_length=MIN_LENGTH,
                  eos_token_id=eos, pad_token_id=1)
        want, got = _state(B, hists, u, "cpu"), _state(B, hists, u, dev)
        wc, wm = _run(logits, want, **kw)
        gc, gm = _run(logits.to(dev), got, **kw)
        assert torch.equal(got["next_tokens"].cpu(), want["next_tokens"])
        assert torch.equal(got["ids_buf"].cpu(), want["ids_buf"])
        assert torch.equal(got["unfinished"].cpu(), want["unfinished"])
        assert torch.equal(gc.cpu(), wc) and torch.equal(gm.cpu(), wm)
        for b in range(B):
            if b == 2:
                continue
            assert (want["next_tokens"][b, 0] == eos) == \
                (LENS[b] >= MIN_LENGTH)


@pytest.mark.parametrize("V", [257, 1000])
def test_boundary_uniforms(dev, V):
    """u = 0 picks the first kept token, the largest float below 1 the last
    one; never a token of zero probability. Rows whose nucleus has no fp64
    margin, or whose last kept token is lost in the rounding of u * mass (the
    answer is then a matter of summation order), are not compared."""
    rows, hists, u, eos = _small_inputs(V, torch.float32)
    B = 16
    rows = rows.clone()
    rows[:, V - 1] = 6.0  # a last token of weight
    lens = torch.tensor(LENS, dtype=torch.int32)
    x, _, _ = ref.sample_token_filter(rows, hists, lens, 1.0, 0, 1.0, 1.0,
                                      MIN_LENGTH, eos)
    top = torch.tensor(1.0).nextafter(torch.tensor(0.0))
    for uval, top_p in itertools.product([0.0, float(top)], [1.0, 0.5]):
        uu = torch.full_like(u, uval)
        assert uu.max() < 1.0
        kw = dict(top_p=top_p, min_length=MIN_LENGTH, eos_token_id=eos)
        want, got = _state(B, hists, uu, "cpu"), _state(B, hists, uu, dev)
        _run(rows, want, **kw)
        _run(rows.to(dev), got, **kw)
        checked = 0
        for b in range(B):
            if b == 2:
                continue
            p, keep, ahead_last, kept_mass, gap_ok = _oracle(x[b].double(), 0,
                                                             top_p)
            kept = keep.nonzero().flatten()
            if not (gap_ok and _nucleus_margin_ok(top_p, ahead_last, kept_mass)
                    and p[kept[-1]] / p[keep].sum() > V * 2.0 ** -23):
                continue
            expect = int(kept[0] if uval == 0.0 else kept[-1])
            assert p[expect] > 0
            assert int(want["next_tokens"][b, 0]) == expect
            assert int(got["next_tokens"][b, 0]) == expect
            checked += 1
        assert checked >= 12, checked


# -- full vocabulary: fp64 bands --------------------------------------------------

@functools.lru_cache(maxsize=None)
def _full_inputs(V, dtype):
    eos = V - 2
    g = torch.Generator().manual_seed(V)
    logits = (3.0 * torch.randn(16, V, generator=g))
    for b in range(16):
        logits[b, (7 * b + 3) % V] = -float("inf")
    hists = torch.stack([_history(V, b) for b in range(16)])
    u = torch.rand(16, T, generator=g)
    return logits.to(dtype), hists, u, eos


def _nucleus_size(q, tp):
    """Tie-inclusive fp64 nucleus size of unrenormalised q for top_p = tp."""
    s = torch.sort(q, descending=True).values
    c = torch.cumsum(s, 0)
    first = torch.searchsorted(-s, -s, right=False)
    ahead = torch.where(first > 0, c[(first - 1).clamp(min=0)],
                        torch.zeros_like(c))
    return int(((ahead <= tp) & (s > 0)).sum())


FULL_CONFIGS = [(0, 0.9, 1.0, 1.0), (0, 0.5, 1.3, 0.7), (40, 0.9, 1.3, 1.0),
                (0, 1.0, 1.0, 0.7)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("V", [50257, 50304])
def test_full_vocab_bands(dev, V, B, dtype):
    _check_bands(dev, V, B, dtype, FULL_CONFIGS)


@pytest.mark.parametrize("V", [4096, 4097, 16384, 16385, 51200, 51201, 65536])
def test_bands_at_kernel_size_steps(dev, V):
    """Both sides of every vocabulary size at which the launcher picks a
    kernel with more slots per thread (4, 16, 50, 64), and the largest V."""
    _check_bands(dev, V, 3, torch.float32, FULL_CONFIGS[2:3])
    logits, hists, u, eos = _full_inputs(V, torch.float32)
    want, got = _state(3, hists, u, "cpu"), _state(3, hists, u, dev)
    kw = dict(greedy=True, repetition_penalty=1.3, eos_token_id=eos,
              pad_token_id=1)
    _run(logits[:3], want, **kw)
    _run(logits[:3].to(dev), got, **kw)
    assert torch.equal(got["next_tokens"].cpu(), want["next_tokens"])


def _check_bands(dev, V, B, dtype, configs):
    logits, hists, u, eos = _full_inputs(V, dtype)
    logits, lens = logits[:B], torch.tensor(LENS[:B], dtype=torch.int32)
    dlogits = logits.to(dev)
    delta = V * 2.0 ** -23
    for top_k, top_p, pen, temp in configs:
        kw = dict(temperature=temp, top_k=top_k, top_p=top_p,
                  repetition_penalty=pen, min_length=MIN_LENGTH,
                  eos_token_id=eos, pad_token_id=1)
        got = _state(B, hists, u, dev)
        gc, gm = _run(dlogits, got, **kw)
        gc, gm, tok = gc.cpu(), gm.cpu(), got["next_tokens"].cpu()[:, 0]
        x, _, _ = ref.sample_token_filter(logits, hists[:B], lens, 1.0, 0,
                                          1.0, pen, MIN_LENGTH, eos)
        z = (x / temp if temp != 1.0 else x).double()
        for b in range(B):
            p = torch.softmax(z[b], dim=-1)
            q = p
            if 0 < top_k < V:
                kth = torch.sort(p, descending=True).values[top_k - 1]
                q = torch.where(p >= kth, p, torch.zeros_like(p))
            n = int(gc[b])
            if top_p < 1.0:
                lo = _nucleus_size(q, top_p - delta)
                hi = _nucleus_size(q, top_p + delta)
            else:
                lo = hi = int((q > 0).sum())
            assert lo <= n <= hi, (b, lo, n, hi)
            # the kernel's kept set: the n most probable tokens (whole ties)
            thr = torch.sort(q, descending=True).values[n - 1]
            keep = (q >= thr) & (q > 0)
            assert int(keep.sum()) == n
            kept = torch.where(keep, q, torch.zeros_like(q))
            cum = torch.cumsum(kept, 0)
            mass = float(cum[-1])
            assert abs(float(gm[b]) - mass) <= delta * mass
            if b == 2:
                assert int(tok[b]) == 1  # finished row: pad
                continue
            v = int(tok[b])
            assert 0 <= v < V and bool(keep[v]) and float(p[v]) > 0
            target = float(u[b, min(LENS[b], T - 1)].double()) * mass
            before = float(cum[v] - kept[v])
            assert before - delta * mass <= target <= \
                float(cum[v]) + delta * mass, (b, v, before, target)


# -- reproducibility and writes ---------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [1000, 50304])
def test_reproducible_and_writes_only_its_slot(dev, V, dtype):
    logits, hists, u, eos = _full_inputs(V, dtype) if V > 1000 else \
        _small_inputs(V, dtype)
    B = 16
    # a strided view: the row stride is not V
    wide = torch.zeros(B, V + 24, dtype=dtype, device=dev)
    wide[:, :V] = logits.to(dev)
    dl = wide[:, :V]
    assert dl.stride(0) == V + 24
    kw = dict(temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=1.3,
              min_length=MIN_LENGTH, eos_token_id=eos, pad_token_id=1)
    a, b = _state(B, hists, u, dev), _state(B, hists, u, dev)
    ac, am = _run(dl, a, **kw)
    bc, bm = _run(dl, b, **kw)
    cc, cm = _run(logits.to(dev), _state(B, hists, u, dev), **kw)
    for k in ("ids_buf", "lens", "unfinished", "next_tokens", "u"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(ac, bc) and torch.equal(ac, cc)
    assert torch.equal(am.view(torch.int32), bm.view(torch.int32))
    assert torch.equal(am.view(torch.int32), cm.view(torch.int32))
    ids = a["ids_buf"].cpu()
    assert a["lens"].cpu().tolist() == LENS  # lens is read only
    for r in range(B):
        changed = (ids[r] != hists[r]).nonzero().flatten().tolist()
        assert changed in ([], [LENS[r]]), (r, changed)
        if LENS[r] < T:
            assert ids[r, LENS[r]] == a["next_tokens"][r, 0].cpu()
    assert torch.equal(ids[15], hists[15])  # the full row is not written


def test_argument_errors_and_fallback(dev):
    V = 300
    logits = torch.randn(2, V, device=dev)
    st = _state(2, torch.zeros(16, T, dtype=torch.long), torch.rand(16, T), dev)
    with pytest.raises(RuntimeError, match="lens"):
        sample_token(logits, st["ids_buf"], st["lens"].long(),
                     st["unfinished"], st["u"], st["next_tokens"])
    with pytest.raises(RuntimeError, match="temperature"):
        sample_token(logits, st["ids_buf"], st["lens"], st["unfinished"],
                     st["u"], st["next_tokens"], temperature=0.0)
    with pytest.raises(RuntimeError, match="u must be"):
        sample_token(logits, st["ids_buf"], st["lens"], st["unfinished"],
                     st["u"][:, :5], st["next_tokens"])
    # past 65536 tokens the op runs the twin, on the device
    big = torch.randn(2, 65537, device=dev)
    big[:, 65536] = 40.0
    sample_token(big, st["ids_buf"], st["lens"], st["unfinished"], st["u"],
                 st["next_tokens"], greedy=True)
    assert st["next_tokens"][:, 0].tolist() == [65536, 65536]
