"""Row kernels at their edges: fp32 I/O, fallback paths, odd shapes, row
loops, offset rows, and the host-side refusals of the bindings.

Every comparison is against a float64 torch computation of the same
formula, written out here (the ``*_ref`` functions). Inputs are rounded to
the kernel dtype first and widened to float64 afterwards, so the reference
sees the values the kernel sees.

Tolerances
----------
bf16 outputs keep the tolerances test_ops_gpu.py uses for the same op
(BF16_TOL); the 2^-8 output rounding dominates them.

fp32 outputs and fp32 statistics (mean, rstd, lse, loss, dw, db, ...) are
not guessed. For each output the same ``*_ref`` formula was run in float32
on the CPU over every input this file uses and compared with its float64
run:
    rel = max |e - r| / |r|   over the large outputs: |r| at least the median
                              magnitude and within 1e-3 of the largest
    abs = max |e - r|         over the other, small outputs
(a relative error means nothing for a softmax tail, or for p - 1 at the label
of a confident row: those are judged by their absolute error)
The kernel gets rtol = 8 * rel and atol = 8 * abs (the 8 covers __expf,
rsqrtf and another summation order). ``PYTHONPATH=. python tests/test_ops_edges_gpu.py``
repeats the measurement on a CPU and prints the table; FP32_TOL below is
its output, rounded up to two digits.

output                         rel       abs      rtol      atol
adamw.m                   1.02e-06  9.83e-08   8.2e-06   7.9e-07
adamw.master              1.31e-07  6.80e-08   1.1e-06   5.5e-07
adamw.v                   3.96e-07  1.00e-08   3.2e-06   8.1e-08
bg.db                     5.98e-07  1.87e-05   4.8e-06   1.5e-04
bg.dx                     1.85e-06  1.72e-06   1.5e-05   1.4e-05
bg.y                      2.05e-07  7.69e-08   1.7e-06   6.2e-07
ce.dlogits                6.80e-06  2.49e-09   5.5e-05   2.0e-08
ce.loss                   6.94e-08  5.99e-06   5.6e-07   4.8e-05
ce.lse                    4.47e-08  6.78e-06   3.6e-07   5.5e-05
colsum.out                2.86e-07  6.94e-06   2.3e-06   5.6e-05
ln.db                     4.67e-07  2.48e-05   3.8e-06   2.0e-04
ln.dw                     6.85e-07  2.85e-05   5.5e-06   2.3e-04
ln.dx                     5.13e-07  3.99e-07   4.2e-06   3.2e-06
ln.mean                   4.59e-07  4.20e-08   3.7e-06   3.4e-07
ln.rstd                   1.48e-07  1.51e-07   1.2e-06   1.3e-06
ln.y                      5.30e-07  4.71e-07   4.3e-06   3.8e-06
lnoff1000_1.dx            2.58e-05  2.46e-05   2.1e-04   2.0e-04
lnoff1000_1.y             2.16e-04  1.61e-04   1.8e-03   1.3e-03
lnoff100_0.25.dx          1.49e-05  3.24e-05   1.2e-04   2.6e-04
lnoff100_0.25.y           1.02e-04  7.78e-05   8.2e-04   6.3e-04
lnoff3_0.01.dx            1.26e-05  8.90e-04   1.1e-04   7.2e-03
lnoff3_0.01.y             8.27e-05  5.90e-05   6.7e-04   4.8e-04
lnoff4096_1.dx            9.76e-05  8.36e-05   7.9e-04   6.7e-04
lnoff4096_1.y             7.10e-04  5.56e-04   5.7e-03   4.5e-03
res.db                    4.67e-07  2.48e-05   3.8e-06   2.0e-04
res.dw                    7.44e-07  2.91e-05   6.0e-06   2.4e-04
res.dx                    5.46e-07  5.91e-07   4.4e-06   4.8e-06
res.mean                  4.26e-07  1.74e-08   3.5e-06   1.4e-07
res.rstd                  1.42e-07  9.05e-08   1.2e-06   7.3e-07
res.y                     4.97e-07  4.11e-07   4.0e-06   3.3e-06
rms.dw                    5.26e-07  2.73e-05   4.3e-06   2.2e-04
rms.dx                    6.20e-07  5.22e-07   5.0e-06   4.2e-06
rms.rstd                  1.45e-07  1.67e-07   1.2e-06   1.4e-06
rms.y                     2.54e-07  1.31e-07   2.1e-06   1.1e-06
rope.dx                   1.52e-07  1.13e-07   1.3e-06   9.1e-07
rope.y                    1.47e-07  1.09e-07   1.2e-06   8.8e-07
smb.dbias                 8.38e-06  1.55e-07   6.8e-05   1.3e-06
smb.ds                    2.48e-05  2.99e-08   2.0e-04   2.4e-07
smb.y                     6.33e-07  4.12e-09   5.1e-06   3.3e-08
smc.ds                    3.94e-06  1.84e-09   3.2e-05   1.5e-08
smc.y                     3.24e-07  8.06e-09   2.6e-06   6.5e-08
smc200.ds                 4.62e-05  1.34e-07   3.7e-04   1.1e-06
smc200.y                  9.37e-08  5.34e-14   7.5e-07   4.3e-13
sumsq.out                 2.42e-08  0.00e+00   2.0e-07   0.0e+00
vp.dlogits                1.07e-06  1.91e-09   8.6e-06   1.6e-08
vp.loss                   6.80e-08  1.93e-06   5.5e-07   1.6e-05
vp.sumexp                 1.76e-07  2.43e-07   1.5e-06   2.0e-06

Sensitivity, shown once with temporary edits of the kernels: a register LN
forward that handles only the first row of each block fails the six
4099x1024 cases of test_norm_fwd_bwd (3 of 4099 means off); a bias scaled
together with the scores, (v + b) * scale, fails every fused scale-0.25
case of test_softmax_bias_edges; a truncated instead of rounded bf16 model
copy fails the bit equality in the four model_bf16 AdamW cases.

Fixed by derivation, not measured: the offset-row LayerNorm bounds (rstd
within 1e-4, mean within 1e-6 relative of float64: about 100x under the
one-pass variance error and 1000x over the two-pass one) and the bit
equality of AdamW's bf16 model copy with the rounded fp32 master.
"""

import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from paddlefleetx_amd.ops import functional as F
from paddlefleetx_amd.ops import hip_ext

DEV = "cuda:0"
BF16, FP32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = [BF16, FP32]
IDS = {BF16: "bf16", FP32: "fp32"}

# (rtol, atol) per output, as test_ops_gpu.py has them for the same op
BF16_TOL = {
    "ln.y": (3e-2, 3e-2), "ln.dx": (5e-2, 5e-2),
    "rms.y": (3e-2, 3e-2), "rms.dx": (5e-2, 5e-2),
    "res.y": (3e-2, 3e-2), "res.dx": (5e-2, 5e-2),
    "lnoff.y": (3e-2, 3e-2), "lnoff.dx": (5e-2, 5e-2),
    "smc.y": (1e-2, 1e-2), "smc.ds": (2e-2, 2e-2),
    "smc200.y": (1e-2, 1e-2), "smc200.ds": (2e-2, 2e-2),
    "smb.y": (1e-2, 1e-2), "smb.ds": (2e-2, 2e-2), "smb.dbias": (2e-2, 2e-2),
    "ce.dlogits": (2e-2, 2e-2), "vp.dlogits": (2e-2, 2e-2),
    "bg.y": (2e-2, 2e-2), "bg.dx": (3e-2, 3e-2),
    "rope.y": (2e-2, 2e-2), "rope.dx": (2e-2, 2e-2),
}
# db of bias_gelu on bf16 sums the ROUNDED bf16 dx: not an fp32-exact sum
BG_DB_BF16 = (1e-2, 0.5)

FP32_TOL = {
    "adamw.m": (8.2e-06, 7.9e-07),
    "adamw.master": (1.1e-06, 5.5e-07),
    "adamw.v": (3.2e-06, 8.1e-08),
    "bg.db": (4.8e-06, 1.5e-04),
    "bg.dx": (1.5e-05, 1.4e-05),
    "bg.y": (1.7e-06, 6.2e-07),
    "ce.dlogits": (5.5e-05, 2.0e-08),
    "ce.loss": (5.6e-07, 4.8e-05),
    "ce.lse": (3.6e-07, 5.5e-05),
    "colsum.out": (2.3e-06, 5.6e-05),
    "ln.db": (3.8e-06, 2.0e-04),
    "ln.dw": (5.5e-06, 2.3e-04),
    "ln.dx": (4.2e-06, 3.2e-06),
    "ln.mean": (3.7e-06, 3.4e-07),
    "ln.rstd": (1.2e-06, 1.3e-06),
    "ln.y": (4.3e-06, 3.8e-06),
    "lnoff1000_1.dx": (2.1e-04, 2.0e-04),
    "lnoff1000_1.y": (1.8e-03, 1.3e-03),
    "lnoff100_0.25.dx": (1.2e-04, 2.6e-04),
    "lnoff100_0.25.y": (8.2e-04, 6.3e-04),
    "lnoff3_0.01.dx": (1.1e-04, 7.2e-03),
    "lnoff3_0.01.y": (6.7e-04, 4.8e-04),
    "lnoff4096_1.dx": (7.9e-04, 6.7e-04),
    "lnoff4096_1.y": (5.7e-03, 4.5e-03),
    "res.db": (3.8e-06, 2.0e-04),
    "res.dw": (6.0e-06, 2.4e-04),
    "res.dx": (4.4e-06, 4.8e-06),
    "res.mean": (3.5e-06, 1.4e-07),
    "res.rstd": (1.2e-06, 7.3e-07),
    "res.y": (4.0e-06, 3.3e-06),
    "rms.dw": (4.3e-06, 2.2e-04),
    "rms.dx": (5.0e-06, 4.2e-06),
    "rms.rstd": (1.2e-06, 1.4e-06),
    "rms.y": (2.1e-06, 1.1e-06),
    "rope.dx": (1.3e-06, 9.1e-07),
    "rope.y": (1.2e-06, 8.8e-07),
    "smb.dbias": (6.8e-05, 1.3e-06),
    "smb.ds": (2.0e-04, 2.4e-07),
    "smb.y": (5.1e-06, 3.3e-08),
    "smc.ds": (3.2e-05, 1.5e-08),
    "smc.y": (2.6e-06, 6.5e-08),
    "smc200.ds": (3.7e-04, 1.1e-06),
    "smc200.y": (7.5e-07, 4.3e-13),
    "sumsq.out": (2.0e-07, 0.0e+00),
    "vp.dlogits": (8.6e-06, 1.6e-08),
    "vp.loss": (5.5e-07, 1.6e-05),
    "vp.sumexp": (1.5e-06, 2.0e-06),
}

_WORST = {}      # key -> worst err/bound seen in this run (printed at the end)
_BASELINE = {}   # key -> [rel, abs] (only filled by the __main__ measurement)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_WORST):
        print(f"\n[edges] {k:24s} worst err/bound = {_WORST[k]:.3g}", end="")
    print()


def _tol(key, got):
    return BF16_TOL[key] if got.dtype == BF16 else FP32_TOL[key]


def _cmp(key, got, want, tol=None):
    """|got - want| <= atol + rtol * |want| elementwise; NaN fails."""
    rtol, atol = tol if tol is not None else _tol(key, got)
    g = got.detach().to("cpu", F64)
    want = want.to(F64)
    assert g.shape == want.shape, (key, g.shape, want.shape)
    if g.numel() == 0:
        return
    err = (g - want).abs()
    bound = atol + rtol * want.abs()
    ratio = float(torch.where(err > 0, err / bound.clamp_min(1e-300),
                              torch.zeros_like(err)).nan_to_num(
                                  nan=float("inf")).max())
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    ok = err <= bound
    assert bool(ok.all()), (
        f"{key}: {int((~ok).sum())}/{ok.numel()} outside rtol={rtol:g} "
        f"atol={atol:g}; max err {float(err.nan_to_num(nan=math.inf).max()):.3e}"
        f" = {ratio:.3g} x bound")


def _note_baseline(key, eager, ref):
    e, r = eager.to(F64).reshape(-1), ref.to(F64).reshape(-1)
    if r.numel() == 0:
        return
    err, mag = (e - r).abs(), r.abs()
    big = mag >= max(float(mag.median()), 1e-3 * float(mag.max()))
    rel = float((err[big] / mag[big].clamp_min(1e-300)).max()) \
        if bool((mag[big] > 0).all()) else 0.0
    small = float(err[~big].max()) if bool((~big).any()) else 0.0
    cur = _BASELINE.setdefault(key, [0.0, 0.0])
    cur[0], cur[1] = max(cur[0], rel), max(cur[1], small)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _dev(inp):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items()}


def _check_op(op, case, dtype, prefix=None, tols=None):
    """Run op's kernels on `case`, compare every output with float64."""
    inp = op.make(case, dtype)
    out = op.run(_dev(inp))
    want = op.ref(inp, F64)
    prefix = prefix or inp.get("_key", op.key)
    for name, w in want.items():
        _cmp(f"{prefix}.{name}", out[name], w, (tols or {}).get(name))
    return inp, out, want


# ---------------------------------------------------------------------------
# LayerNorm / RMSNorm / residual LayerNorm
# ---------------------------------------------------------------------------

LN_SHAPES = [
    (33, 1000),                       # generic VEC=4
    (33, 3072), (5, 32),              # generic VEC=8; 32: most threads idle
    (4099, 1024),                     # register path, grid=4096: 3 blocks x 2 rows
    (4099, 32),                       # same loop in the fallback
    (3, 2048), (3, 4096), (3, 5120), (3, 8192),   # every LN_FOR_EACH_SHAPE
    (15, 1024), (16, 1024), (17, 1024), (33, 1024),  # rows_per_chunk=16 edges
]
RES_SHAPES = [(33, 1000), (4099, 1024)]


def _ln_make(case, dtype):
    kind, (N, H) = case
    g = _g(1000 + 7 * N + H)
    r = lambda *s: torch.randn(*s, generator=g)
    inp = dict(kind=kind, eps=1e-6 if kind == "rms" else 1e-5,
               x=r(N, H).to(dtype), w=(1 + 0.5 * r(H)).to(dtype),
               b=(0.5 * r(H)).to(dtype), dy=r(N, H).to(dtype), _key=kind)
    if kind == "res":
        inp["res"] = r(N, H).to(dtype)
        inp["dsum"] = r(N, H).to(dtype)
    return inp


def _ln_ref(inp, dt):
    kind, eps = inp["kind"], inp["eps"]
    out = {}
    if kind == "res":
        # fp32 add then round-to-nearest-even: bit for bit what the kernel
        # stores and then normalises
        s = (inp["x"].float() + inp["res"].float()).to(inp["x"].dtype)
        out["s"] = s
        x = s.to(dt)
    else:
        x = inp["x"].to(dt)
    w, b, dy = inp["w"].to(dt), inp["b"].to(dt), inp["dy"].to(dt)
    if kind == "rms":
        mu = torch.zeros(x.shape[0], dtype=dt)
        var = (x * x).mean(1)
    else:
        mu = x.mean(1)
        var = ((x - mu[:, None]) ** 2).mean(1)   # two-pass, as torch does
        out["mean"] = mu
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu[:, None]) * rstd[:, None]
    out["rstd"] = rstd
    out["y"] = xh * w if kind == "rms" else xh * w + b
    gw = dy * w
    c2 = (gw * xh).mean(1)
    if kind == "rms":
        dx = (gw - xh * c2[:, None]) * rstd[:, None]
    else:
        dx = (gw - gw.mean(1)[:, None] - xh * c2[:, None]) * rstd[:, None]
        out["db"] = dy.sum(0)
    if kind == "res":
        dx = dx + inp["dsum"].to(dt)
    out["dx"] = dx
    out["dw"] = (dy * xh).sum(0)
    return out


def _ln_run(i):
    ext, kind = hip_ext(), i["kind"]
    if kind == "rms":
        y, rstd = ext.rmsnorm_fwd(i["x"], i["w"], i["eps"])
        dx, dw = ext.rmsnorm_bwd(i["dy"], i["x"], i["w"], rstd)
        return dict(y=y, rstd=rstd, dx=dx, dw=dw)
    if kind == "ln":
        y, mean, rstd = ext.layernorm_fwd(i["x"], i["w"], i["b"], i["eps"])
        dx, dw, db = ext.layernorm_bwd(i["dy"], i["x"], i["w"], mean, rstd)
        return dict(y=y, mean=mean, rstd=rstd, dx=dx, dw=dw, db=db)
    y, mean, rstd, s = ext.layernorm_fwd_residual(i["x"], i["res"], i["w"],
                                                  i["b"], i["eps"])
    dx, dw, db = ext.layernorm_bwd_residual(i["dy"], s, i["w"], mean, rstd,
                                            i["dsum"])
    return dict(y=y, mean=mean, rstd=rstd, s=s, dx=dx, dw=dw, db=db)


LN = SimpleNamespace(
    key="ln", make=_ln_make, ref=_ln_ref, run=_ln_run,
    cases=[("ln", s) for s in LN_SHAPES] + [("rms", s) for s in LN_SHAPES]
    + [("res", s) for s in RES_SHAPES])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", LN.cases, ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}")
def test_norm_fwd_bwd(case, dtype):
    # the stored residual sum must be the rounded fp32 sum, bit for bit
    _check_op(LN, case, dtype, tols={"s": (0.0, 0.0)})


# rows drawn as mean + std * randn: the one-pass variance E[x^2] - mu^2 lost
# 1e-2 .. all of rstd on these (NaN at mean 4096), the two-pass one ~1e-7
OFFSETS = [(FP32, 1000.0, 1.0), (FP32, 4096.0, 1.0), (FP32, 100.0, 0.25),
           (FP32, 3.0, 0.01), (BF16, 1000.0, 1.0), (BF16, 100.0, 0.25)]


def _off_make(case, dtype):
    (_, mean, std), H = case
    g = _g(77 + H + int(mean))
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(kind="ln", eps=1e-5, x=(mean + std * r(64, H)).to(dtype),
                w=(1 + 0.1 * r(H)).to(dtype), b=(0.1 * r(H)).to(dtype),
                dy=r(64, H).to(dtype), _key=f"lnoff{mean:g}_{std:g}")


LNOFF = SimpleNamespace(key="lnoff", make=_off_make, ref=_ln_ref, run=_ln_run,
                        cases=[(o, H) for o in OFFSETS for H in (1024, 1000)])


@pytest.mark.parametrize(
    "case", LNOFF.cases,
    ids=lambda c: f"{IDS[c[0][0]]}-mean{c[0][1]:g}-std{c[0][2]:g}-H{c[1]}")
def test_layernorm_offset_rows(case):
    """Fails on the one-pass variance (rstd off by >= 5e-3, or NaN)."""
    dtype = case[0][0]
    inp = LNOFF.make(case, dtype)
    out = LNOFF.run(_dev(inp))
    want = LNOFF.ref(inp, F64)
    for name in ("y", "mean", "rstd", "dx", "dw", "db"):
        assert bool(torch.isfinite(out[name]).all()), f"{name} is not finite"
    rstd_err = float(((out["rstd"].cpu().double() - want["rstd"]).abs()
                      / want["rstd"]).max())
    mean_err = float(((out["mean"].cpu().double() - want["mean"]).abs()
                      / want["mean"].abs()).max())
    print(f"\n[edges] offset {inp['_key']} H={case[1]}: rstd rel err "
          f"{rstd_err:.3e}, mean rel err {mean_err:.3e}", end="")
    assert rstd_err <= 1e-4, rstd_err
    assert mean_err <= 1e-6, mean_err
    if dtype == BF16:
        _cmp("lnoff.y", out["y"], want["y"])
        _cmp("lnoff.dx", out["dx"], want["dx"])
    else:
        _cmp(inp["_key"] + ".y", out["y"], want["y"])
        _cmp(inp["_key"] + ".dx", out["dx"], want["dx"])


# ---- wrappers: fp32 parameters on bf16 activations, strided x ----

def _wrapper_inputs(N, H, seed):
    g = _g(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(N, H).to(BF16), res=r(N, H).to(BF16), w=1 + 0.5 * r(H),
                b=0.5 * r(H), dy=r(N, H).to(BF16), dsum=r(N, H).to(BF16))


@pytest.mark.parametrize("kind", ["ln", "res", "rms"])
def test_norm_wrappers_fp32_params_on_bf16(kind):
    """fp32 weights are cast to bf16 before the kernel (which would read
    their buffer as bf16 otherwise); grads come back in fp32."""
    c = _wrapper_inputs(33, 1024, 5)
    d = _dev(c)
    x = d["x"].clone().requires_grad_(True)
    res = d["res"].clone().requires_grad_(True)
    w = d["w"].clone().requires_grad_(True)
    b = d["b"].clone().requires_grad_(True)
    eps = 1e-6 if kind == "rms" else 1e-5
    if kind == "ln":
        y = F.layernorm(x, w, b, eps)
        y.backward(d["dy"])
    elif kind == "rms":
        y = F.rmsnorm(x, w, eps)
        y.backward(d["dy"])
    else:
        y, s = F.layernorm_residual(x, res, w, b, eps)
        torch.autograd.backward([y, s], [d["dy"], d["dsum"]])
    # the reference sees the bf16-rounded parameters, as the kernel does
    inp = dict(kind=kind, eps=eps, x=c["x"], res=c["res"], dy=c["dy"],
               dsum=c["dsum"], w=c["w"].to(BF16), b=c["b"].to(BF16))
    want = _ln_ref(inp, F64)
    assert y.dtype == BF16
    _cmp(f"{kind}.y", y, want["y"])
    _cmp(f"{kind}.dx", x.grad, want["dx"])
    assert w.grad.dtype == FP32
    _cmp(f"{kind}.dw", w.grad, want["dw"])
    if kind != "rms":
        assert b.grad.dtype == FP32
        _cmp(f"{kind}.db", b.grad, want["db"])
    if kind == "res":
        assert torch.equal(s.cpu(), want["s"])
        assert torch.equal(res.grad, x.grad)


def test_fused_layernorm_module_bf16_input_and_strided_x():
    c = _wrapper_inputs(40, 1024, 6)
    mod = F.FusedLayerNorm(1024).to(DEV)
    assert mod.weight.dtype == FP32
    with torch.no_grad():
        mod.weight.copy_(c["w"])
        mod.bias.copy_(c["b"])
    # x is a transposed view: the wrapper has to make it contiguous itself
    base = c["x"].t().contiguous().to(DEV)           # [H, N]
    x = base.t().requires_grad_(True)                # [N, H], strides (1, N)
    assert not x.is_contiguous()
    y = mod(x)
    y.backward(c["dy"].to(DEV))
    inp = dict(kind="ln", eps=1e-5, x=c["x"], dy=c["dy"], w=c["w"].to(BF16),
               b=c["b"].to(BF16))
    want = _ln_ref(inp, F64)
    _cmp("ln.y", y, want["y"])
    _cmp("ln.dx", x.grad, want["dx"])
    assert mod.weight.grad.dtype == FP32 and mod.bias.grad.dtype == FP32
    _cmp("ln.dw", mod.weight.grad, want["dw"])
    _cmp("ln.db", mod.bias.grad, want["db"])


# ---------------------------------------------------------------------------
# Softmax
# ---------------------------------------------------------------------------

SMC_CASES = [((1, 2, 5, 5), 1), ((1, 1, 1, 300), 1), ((2, 2, 7, 263), 1),
             ((1, 2, 257, 257), 1), ((2, 2, 7, 263), 200)]


def _causal_mask(Sq, Sk):
    i = torch.arange(Sq)[:, None]
    j = torch.arange(Sk)[None, :]
    return j <= i + (Sk - Sq)


def _smc_make(case, dtype):
    shape, mult = case
    g = _g(300 + shape[2] + shape[3] + mult)
    # x200 with scale 1: exp(600) overflows unless the row max is subtracted
    return dict(s=(mult * torch.randn(*shape, generator=g)).to(dtype),
                dy=torch.randn(*shape, generator=g).to(dtype),
                scale=1.0 if mult > 1 else 0.5,
                _key="smc200" if mult > 1 else "smc")


def _smc_ref(inp, dt):
    s, dy, scale = inp["s"].to(dt), inp["dy"].to(dt), inp["scale"]
    mask = _causal_mask(s.shape[2], s.shape[3])
    z = (s * scale).masked_fill(~mask, float("-inf"))
    y = torch.softmax(z, -1)
    ds = y * (dy - (dy * y).sum(-1, keepdim=True)) * scale
    return dict(y=y, ds=ds)


def _smc_run(i):
    y = hip_ext().softmax_causal_fwd(i["s"], i["scale"])
    ds = hip_ext().softmax_causal_bwd(i["dy"], y, i["scale"])
    return dict(y=y, ds=ds)


SMC = SimpleNamespace(key="smc", make=_smc_make, ref=_smc_ref, run=_smc_run,
                      cases=SMC_CASES)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", SMC_CASES,
                         ids=lambda c: "x".join(map(str, c[0])) + f"-x{c[1]}")
def test_softmax_causal_edges(case, dtype):
    inp, out, _ = _check_op(SMC, case, dtype)
    y = out["y"].cpu()
    mask = _causal_mask(y.shape[2], y.shape[3]).expand_as(y)
    assert bool((y[~mask] == 0).all()), "masked positions must be exactly 0"
    assert bool(torch.isfinite(y).all())
    # every stored element is off by at most the unit roundoff of its dtype
    # (2^-8 relative for bf16), and so is the row sum; the fp32 sum before
    # rounding is 1 up to the reduction and division error of a 300-term
    # fp32 row, (log2(300) + 3) * 2^-24 < 2^-20
    bound = 2.0 ** -8 if dtype == BF16 else 2.0 ** -20
    dev = float((y.double().sum(-1) - 1).abs().max())
    assert dev <= bound, dev


SMB_SHAPE = (2, 3, 2, 5, 37)
SMB_BIAS = [(2, 1, 2, 5, 37), (1, 1, 2, 5, 37), (2, 3, 1, 5, 37),
            (2, 3, 2, 5, 37),
            (2, 1, 2, 1, 37)]     # two broadcast runs: torch fallback
SMB_CASES = [(b, sc) for b in SMB_BIAS for sc in (1.0, 0.25)]


def _smb_make(case, dtype):
    bshape, scale = case
    g = _g(500 + sum(bshape))
    return dict(s=(2 * torch.randn(*SMB_SHAPE, generator=g)).to(dtype),
                bias=torch.randn(*bshape, generator=g).to(dtype),
                dy=torch.randn(*SMB_SHAPE, generator=g).to(dtype),
                scale=scale)


def _smb_ref(inp, dt):
    s, bias, dy = inp["s"].to(dt), inp["bias"].to(dt), inp["dy"].to(dt)
    y = torch.softmax(s * inp["scale"] + bias, -1)
    dz = y * (dy - (dy * y).sum(-1, keepdim=True))
    red = [d for d, (a, b) in enumerate(zip(s.shape, bias.shape))
           if b == 1 and a != 1]
    dbias = dz.sum(dim=red, keepdim=True) if red else dz
    return dict(y=y, ds=dz * inp["scale"], dbias=dbias)


def _smb_run(i):
    s = i["s"].clone().requires_grad_(True)
    bias = i["bias"].clone().requires_grad_(True)
    y = F.fused_softmax_bias(s, bias, i["scale"])
    y.backward(i["dy"])
    return dict(y=y, ds=s.grad, dbias=bias.grad)


SMB = SimpleNamespace(key="smb", make=_smb_make, ref=_smb_ref, run=_smb_run,
                      cases=SMB_CASES)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize(
    "case", SMB_CASES, ids=lambda c: "x".join(map(str, c[0])) + f"-s{c[1]}")
def test_softmax_bias_edges(case, dtype):
    inp, out, want = _check_op(SMB, case, dtype)
    period = F._bias_period(SMB_SHAPE, case[0])
    if case[0] == SMB_BIAS[-1]:
        assert period is None       # the wrapper took the torch fallback
        return
    # the binding itself, with the periods the wrapper computed
    d = _dev(inp)
    y = hip_ext().softmax_bias_fwd(d["s"], d["bias"].contiguous(), period[0],
                                   period[1], inp["scale"])
    assert torch.equal(y, out["y"])
    _cmp("smb.y", y, want["y"])


# ---------------------------------------------------------------------------
# Cross entropy and the vocab-parallel helpers
# ---------------------------------------------------------------------------

CE_CASES = [(1, -100), (2, -100), (255, -100), (256, -100), (257, -1),
            (1000, -100)]
CE_N = 19


def _ce_labels(g, N, V, ignore, extra=()):
    lab = torch.randint(0, V, (N,), generator=g)
    fixed = [0, V - 1, ignore, *extra]
    lab[:len(fixed)] = torch.tensor(fixed)
    lab[N - 1] = ignore
    return lab


def _ce_make(case, dtype):
    V, ignore = case
    g = _g(700 + V)
    return dict(logits=(50 * torch.randn(CE_N, V, generator=g)).to(dtype),
                labels=_ce_labels(g, CE_N, V, ignore),
                dloss=torch.randn(CE_N, generator=g), ignore=ignore)


def _ce_ref(inp, dt):
    x, lab, dloss = inp["logits"].to(dt), inp["labels"], inp["dloss"].to(dt)
    valid = lab != inp["ignore"]
    safe = lab.masked_fill(~valid, 0)
    lse = torch.logsumexp(x, 1)
    picked = x.gather(1, safe[:, None]).squeeze(1)
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse))
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x).scatter_(1, safe[:, None], 1.0)
    dl = (p - onehot) * (dloss * valid)[:, None]
    return dict(lse=lse, loss=loss, dlogits=dl)


def _ce_run(i):
    ext = hip_ext()
    loss, lse = ext.cross_entropy_fwd(i["logits"], i["labels"], i["ignore"])
    dl = ext.cross_entropy_bwd(i["dloss"], i["logits"], i["labels"], lse,
                               i["ignore"])
    return dict(lse=lse, loss=loss, dlogits=dl)


CE = SimpleNamespace(key="ce", make=_ce_make, ref=_ce_ref, run=_ce_run,
                     cases=CE_CASES)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", CE_CASES, ids=lambda c: f"V{c[0]}-ign{c[1]}")
def test_cross_entropy_edges(case, dtype):
    inp, out, _ = _check_op(CE, case, dtype)
    ignored = (inp["labels"] == inp["ignore"]).to(DEV)
    assert int(ignored.sum()) >= 2
    assert bool((out["loss"][ignored] == 0).all())
    assert bool((out["dlogits"][ignored] == 0).all())
    assert bool(torch.isfinite(out["dlogits"]).all())


VP_V = 1000
VP_WIDTHS = {2: (333, 667), 3: (100, 512, 388)}


def _vp_make(case, dtype):
    P = case
    g = _g(900 + P)
    edges = []
    start = 0
    for wdt in VP_WIDTHS[P]:
        edges += [start, start + wdt - 1]
        start += wdt
    return dict(logits=(8 * torch.randn(CE_N, VP_V, generator=g)).to(dtype),
                labels=_ce_labels(g, CE_N, VP_V, -100, edges),
                dloss=torch.randn(CE_N, generator=g), ignore=-100, P=P)


def _vp_ref(inp, dt):
    out = _ce_ref(inp, dt)
    x, lab = inp["logits"].to(dt), inp["labels"]
    valid = lab != inp["ignore"]
    gmax = x.max(1).values
    picked = x.gather(1, lab.masked_fill(~valid, 0)[:, None]).squeeze(1)
    return dict(gmax=gmax, sumexp=torch.exp(x - gmax[:, None]).sum(1),
                picked=picked * valid, loss=out["loss"],
                dlogits=out["dlogits"])


def _vp_run(i):
    """What parallel/tp.py does across ranks, with the all-reduces replaced
    by a max / sum over the shards of one device."""
    ext = hip_ext()
    shards = [s.contiguous() for s in i["logits"].split(VP_WIDTHS[i["P"]], 1)]
    starts = [0]
    for s in shards[:-1]:
        starts.append(starts[-1] + s.shape[1])
    lab, ign = i["labels"], i["ignore"]
    gmax = torch.stack([ext.row_max(s) for s in shards]).max(0).values
    sumexp = torch.stack([ext.row_sumexp(s, gmax) for s in shards]).sum(0)
    picked = torch.stack([ext.gather_label_logit(s, lab, st, ign)
                          for s, st in zip(shards, starts)]).sum(0)
    lse = torch.log(sumexp) + gmax
    loss = torch.where(lab != ign, lse - picked, torch.zeros_like(lse))
    dl = torch.cat([ext.vp_ce_bwd(i["dloss"], s, lab, lse, st, ign)
                    for s, st in zip(shards, starts)], 1)
    return dict(gmax=gmax, sumexp=sumexp, picked=picked, loss=loss,
                dlogits=dl)


VP = SimpleNamespace(key="vp", make=_vp_make, ref=_vp_ref, run=_vp_run,
                     cases=[2, 3])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("P", [2, 3])
def test_vocab_parallel_helpers(P, dtype):
    # a max and a single picked logit involve no rounding at all
    inp, out, _ = _check_op(VP, P, dtype,
                            tols={"gmax": (0.0, 0.0), "picked": (0.0, 0.0)})
    ignored = (inp["labels"] == -100).to(DEV)
    assert bool((out["dlogits"][ignored] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_gather_label_logit_second_block(dtype):
    """N = 257: one row lands in the second 256-thread block."""
    g = _g(41)
    N, V, start = 257, 13, 5
    x = torch.randn(N, V, generator=g).to(dtype)
    lab = torch.randint(0, start + V + 6, (N,), generator=g)
    lab[0], lab[1], lab[2], lab[256] = start, start + V - 1, -100, start + 3
    got = hip_ext().gather_label_logit(x.to(DEV), lab.to(DEV), start, -100)
    inside = (lab >= start) & (lab < start + V)
    want = x.double().gather(1, (lab - start).clamp(0, V - 1)[:, None]) \
        .squeeze(1) * inside
    assert got.dtype == FP32
    _cmp("gather", got, want, (0.0, 0.0))


# ---------------------------------------------------------------------------
# bias_gelu, colsum, grad_sumsq, adamw_flat, rope
# ---------------------------------------------------------------------------

GELU_K = math.sqrt(2.0 / math.pi)
BG_SPECIALS = [30.0, -30.0, 0.0, 1e-3, -1e-3, 5.0, -5.0, 2e-3]
BG_CASES = [(N, H, hb) for (N, H) in [(37, 4), (37, 12), (37, 8), (16387, 8)]
            for hb in (True, False)]


def _bg_make(case, dtype):
    N, H, has_bias = case
    g = _g(1100 + N + H)
    x = 3 * torch.randn(N, H, generator=g)
    # +-30 saturate the exp-based tanh, ~1e-3 is its small-argument end
    x.view(-1)[:len(BG_SPECIALS)] = torch.tensor(BG_SPECIALS)
    return dict(x=x.to(dtype), dy=torch.randn(N, H, generator=g).to(dtype),
                bias=(0.5 * torch.randn(H, generator=g)).to(dtype)
                if has_bias else None)


def _bg_ref(inp, dt):
    v, dy = inp["x"].to(dt), inp["dy"].to(dt)
    if inp["bias"] is not None:
        v = v + inp["bias"].to(dt)
    t = torch.tanh(GELU_K * (v + 0.044715 * v ** 3))
    dgelu = 0.5 * (1 + t) + 0.5 * v * (1 - t * t) * GELU_K * (
        1 + 3 * 0.044715 * v * v)
    out = dict(y=0.5 * v * (1 + t), dx=dy * dgelu)
    if inp["bias"] is not None:
        out["db"] = out["dx"].sum(0)
    return out


def _bg_run(i):
    x = i["x"].clone().requires_grad_(True)
    bias = None if i["bias"] is None else i["bias"].clone().requires_grad_(True)
    y = F.bias_gelu(x, bias)
    y.backward(i["dy"])
    out = dict(y=y, dx=x.grad)
    if bias is not None:
        # the binding's own fp32 column sum, before the wrapper's cast
        out["db"] = hip_ext().bias_gelu_bwd(i["dy"], i["x"], i["bias"])[1]
        assert bias.grad.dtype == bias.dtype and out["db"].dtype == FP32
    return out


BG = SimpleNamespace(key="bg", make=_bg_make, ref=_bg_ref, run=_bg_run,
                     cases=BG_CASES)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize(
    "case", BG_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{'bias' if c[2] else 'nobias'}")
def test_bias_gelu_edges(case, dtype):
    _, out, _ = _check_op(BG, case, dtype,
                          tols={"db": BG_DB_BF16} if dtype == BF16 else None)
    assert bool(torch.isfinite(out["y"]).all())
    assert bool(torch.isfinite(out["dx"]).all())


def test_bias_gelu_wrapper_fp32_bias_on_bf16():
    inp = _bg_make((37, 8, True), BF16)
    bias32 = inp["bias"].float() + 1e-4       # not representable in bf16
    x = inp["x"].to(DEV).requires_grad_(True)
    bias = bias32.to(DEV).requires_grad_(True)
    y = F.bias_gelu(x, bias)
    y.backward(inp["dy"].to(DEV))
    want = _bg_ref(dict(inp, bias=bias32.to(BF16)), F64)
    _cmp("bg.y", y, want["y"])
    _cmp("bg.dx", x.grad, want["dx"])
    assert bias.grad.dtype == FP32
    _cmp("bg.db", bias.grad, want["db"], BG_DB_BF16)


COLSUM_SHAPES = [(31, 4), (33, 1028), (4099, 8)]


def _colsum_make(case, dtype):
    return dict(x=torch.randn(*case, generator=_g(1300 + case[0])).to(dtype))


COLSUM = SimpleNamespace(
    key="colsum", make=_colsum_make, cases=COLSUM_SHAPES,
    ref=lambda inp, dt: dict(out=inp["x"].to(dt).sum(0)),
    run=lambda i: dict(out=hip_ext().colsum(i["x"])))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", COLSUM_SHAPES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_colsum_edges(case, dtype):
    _, out, _ = _check_op(COLSUM, case, dtype)
    assert out["out"].dtype == FP32


# one element more than the 2048-block grid covers in one sweep
BIG_N = 2048 * 256 * 4 + 4096


def _sumsq_make(case, dtype):
    return dict(x=torch.randn(BIG_N, generator=_g(1500)).to(dtype))


SUMSQ = SimpleNamespace(
    key="sumsq", make=_sumsq_make, cases=[None],
    ref=lambda inp, dt: dict(
        out=torch.tensor(3.5, dtype=dt) + (inp["x"].to(dt) ** 2).sum()),
    run=None)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_grad_sumsq_grid_stride(dtype):
    """Found by this test: with one fp32 atomicAdd per block (2048 of them
    onto a total of 2.1e6) the bf16 case was 1.99 off, 9.5e-7 relative and
    4.7x the bound below; the kernel now adds the block partials in double
    and updates the slot once (0.12x the bound)."""
    inp = _sumsq_make(None, dtype)
    out = torch.tensor([1.0, 3.5, -2.0], device=DEV)
    hip_ext().grad_sumsq(inp["x"].to(DEV), out, 1)
    # accumulates into the non-zero slot, leaves its neighbours alone
    assert float(out[0]) == 1.0 and float(out[2]) == -2.0
    _cmp("sumsq.out", out[1], SUMSQ.ref(inp, F64)["out"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_grad_sumsq_nonfinite_in_strided_tail(bad, dtype):
    x = torch.ones(BIG_N, device=DEV, dtype=dtype)
    x[BIG_N - 1000] = bad            # only the second sweep of the grid sees it
    out = torch.zeros(2, device=DEV)
    hip_ext().grad_sumsq(x, out, 0)
    if math.isnan(bad):
        assert bool(torch.isnan(out[0]))
    else:
        assert bool(torch.isinf(out[0]))
    assert float(out[1]) == 0.0


ADAMW_COMBOS = [(BF16, BF16), (BF16, FP32), (FP32, BF16), (FP32, FP32),
                (None, FP32)]                     # (model copy, grad)
# (n, step, weight decay)
ADAMW_RUNS = [(4, 1, 0.0), (BIG_N, 100000, 0.01)]
ADAMW_HP = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8)


def _adamw_make(case, dtype=None):
    (model_dt, grad_dt), (n, step, wd) = case
    g = _g(1700 + n % 1000)
    r = lambda: torch.randn(n, generator=g)
    return dict(master=r(), grad=r().to(grad_dt), m=0.1 * r(),
                v=0.01 * r().abs(), step=step, wd=wd, model_dt=model_dt)


def _adamw_ref(inp, dt):
    h = ADAMW_HP
    p, g = inp["master"].to(dt), inp["grad"].to(dt)
    m, v = inp["m"].to(dt), inp["v"].to(dt)
    b1, b2 = torch.tensor(h["b1"], dtype=dt), torch.tensor(h["b2"], dtype=dt)
    bc1, bc2 = 1 - b1 ** inp["step"], 1 - b2 ** inp["step"]
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p * (1 - h["lr"] * inp["wd"])
    p = p - h["lr"] * (m / bc1) / (torch.sqrt(v / bc2) + h["eps"])
    return dict(master=p, m=m, v=v)


def _adamw_run(i):
    h = ADAMW_HP
    n = i["master"].numel()
    model = torch.Tensor() if i["model_dt"] is None else \
        torch.full((n,), 7.0, device=DEV, dtype=i["model_dt"])
    master, m, v = i["master"].clone(), i["m"].clone(), i["v"].clone()
    hip_ext().adamw_flat(master, i["grad"], m, v, model, h["lr"], h["b1"],
                         h["b2"], h["eps"], i["wd"], i["step"])
    return dict(master=master, m=m, v=v, model=model)


ADAMW = SimpleNamespace(
    key="adamw", make=_adamw_make, ref=_adamw_ref, run=_adamw_run,
    cases=[((None, FP32), r) for r in ADAMW_RUNS])


@pytest.mark.parametrize("run", ADAMW_RUNS, ids=lambda r: f"n{r[0]}-step{r[1]}-wd{r[2]}")
@pytest.mark.parametrize(
    "combo", ADAMW_COMBOS,
    ids=lambda c: f"model_{IDS.get(c[0], 'none')}-grad_{IDS[c[1]]}")
def test_adamw_flat_edges(combo, run):
    inp = _adamw_make((combo, run))
    out = _adamw_run(_dev(inp))
    want = _adamw_ref(inp, F64)
    for name in ("master", "m", "v"):      # whole buffers: the tail included
        _cmp(f"adamw.{name}", out[name], want[name])
    if combo[0] == BF16:
        # round-to-nearest-even cast of the UPDATED fp32 master, bit for bit
        assert torch.equal(out["model"], out["master"].to(BF16))
    elif combo[0] == FP32:
        assert torch.equal(out["model"], out["master"])


ROPE_SHAPES = [(1, 2, 4100, 8),     # 8200 rows: past the 8192-block grid
               (2, 3, 5, 2)]        # D = 2: one pair per row


def _rope_make(case, dtype):
    B, H, S, D = case
    g = _g(1900 + S)
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D))
    freqs = torch.outer(torch.arange(S).float(), inv)
    return dict(x=torch.randn(*case, generator=g).to(dtype),
                dy=torch.randn(*case, generator=g).to(dtype),
                cos=freqs.cos().contiguous(), sin=freqs.sin().contiguous())


def _rope_apply(x, cos, sin):
    x1, x2 = x[..., 0::2], x[..., 1::2]
    return torch.stack((x1 * cos - x2 * sin, x2 * cos + x1 * sin), -1).flatten(-2)


def _rope_ref(inp, dt):
    cos, sin = inp["cos"].to(dt), inp["sin"].to(dt)
    # the transpose of a rotation is the rotation by -angle
    return dict(y=_rope_apply(inp["x"].to(dt), cos, sin),
                dx=_rope_apply(inp["dy"].to(dt), cos, -sin))


def _rope_run(i):
    x = i["x"].clone().requires_grad_(True)
    y = F.rope(x, i["cos"], i["sin"])
    y.backward(i["dy"])
    return dict(y=y, dx=x.grad)


ROPE = SimpleNamespace(key="rope", make=_rope_make, ref=_rope_ref,
                       run=_rope_run, cases=ROPE_SHAPES)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("case", ROPE_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_rope_edges(case, dtype):
    _check_op(ROPE, case, dtype)


# ---------------------------------------------------------------------------
# topp_select with explicit u
# ---------------------------------------------------------------------------

TOPP_P = [0.0, 0.5, 1.0, 1.0]      # per row; row 3 is one-hot
_TOPP_ALLOWANCE_USED = []


def _topp_probs(V):
    g = _g(2100 + V)
    p = torch.softmax(torch.randn(4, V, generator=g).double(), -1).float()
    p[3] = 0
    p[3, (7 * V) // 11] = 1.0
    return p


def _topp_pick(sorted_p, top_p, u, dt):
    """Nucleus = shortest prefix whose cumulative sum reaches top_p (all of
    the row if it never does); pick = first index whose cumulative sum
    reaches u * mass(nucleus). Returns (pick, cumsum, target) per row."""
    cum = torch.cumsum(sorted_p.to(dt), -1)
    picks, targets = [], []
    for b in range(sorted_p.shape[0]):
        hit = (cum[b] >= torch.tensor(top_p[b], dtype=dt)).nonzero()
        ncut = int(hit[0]) + 1 if hit.numel() else cum.shape[1]
        target = torch.tensor(u, dtype=dt) * cum[b, ncut - 1]
        hit = (cum[b, :ncut] >= target).nonzero()
        picks.append(int(hit[0]) if hit.numel() else ncut - 1)
        targets.append(float(target))
    return picks, cum, targets


@pytest.mark.parametrize("u", [0.0, 0.5, 0.999999])
@pytest.mark.parametrize("V", [1, 255, 256, 257, 1000])
def test_topp_select_explicit_u(V, u):
    probs = _topp_probs(V)
    sorted_p, sorted_idx = torch.sort(probs, dim=-1, descending=True)
    want, cum, targets = _topp_pick(sorted_p, TOPP_P, u, F64)
    # an fp32 scan makes the same picks: the tie allowance below is idle
    assert _topp_pick(sorted_p, TOPP_P, u, FP32)[0] == want
    ids, pp = hip_ext().topp_select(
        sorted_p.to(DEV), sorted_idx.to(DEV),
        torch.tensor(TOPP_P, device=DEV), torch.full((4,), u, device=DEV))
    assert ids.shape == (4, 1) and pp.shape == (4, 1)
    for b in range(4):
        got = int((sorted_idx[b] == int(ids[b, 0])).nonzero()[0])
        assert float(pp[b, 0]) == float(sorted_p[b, got])
        if got != want[b]:
            # fp32 scan tie: the kernel's pick must cross the threshold
            # within 1e-6 in float64, and at most one case may need this
            lo = float(cum[b, got - 1]) if got else 0.0
            assert float(cum[b, got]) >= targets[b] - 1e-6 and \
                lo < targets[b] + 1e-6, (b, got, want[b])
            _TOPP_ALLOWANCE_USED.append((V, u, b))
    assert len(_TOPP_ALLOWANCE_USED) <= 1, _TOPP_ALLOWANCE_USED
    # top_p = 0 keeps the arg-max alone; a one-hot row returns its index
    assert int(ids[0, 0]) == int(probs[0].argmax())
    assert int(ids[3, 0]) == (7 * V) // 11


# ---------------------------------------------------------------------------
# MoE dispatch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["random", "all_dropped", "one_expert"])
@pytest.mark.parametrize("D", [36, 40])          # VEC=4 / VEC=8 row copies
def test_moe_dispatch_edges(D, mode):
    T, E, K = 67, 5, 1
    g = _g(2300 + D)
    x = torch.randn(T, D, generator=g).to(DEV)          # fp32 rows
    ids = torch.randint(0, E, (T * K,), generator=g)
    if mode == "random":
        ids[torch.rand(T * K, generator=g) < 0.2] = -1
    elif mode == "all_dropped":
        ids[:] = -1
    else:
        ids[:] = 3
    ids = ids.to(DEV)
    disp, sel_sorted, counts = hip_ext().moe_dispatch(x, ids, E, K)
    sel = (ids >= 0).nonzero(as_tuple=True)[0]
    ref_counts = torch.bincount(ids[sel], minlength=E)
    assert torch.equal(counts.cpu(), ref_counts.cpu())
    assert disp.shape == (int(ref_counts.sum()), D) and disp.dtype == FP32
    assert torch.equal(disp, x[sel_sorted // K])
    assert torch.equal(sel_sorted.sort().values, sel)    # each slot once
    off = torch.cumsum(ref_counts, 0) - ref_counts
    seg_of_pos = torch.bucketize(
        torch.arange(disp.shape[0], device=DEV), off, right=True) - 1
    assert torch.equal(ids[sel_sorted], seg_of_pos)


# ---------------------------------------------------------------------------
# Refusals: raised on the host, nothing is launched
# ---------------------------------------------------------------------------

def _refusal_calls():
    """name -> (binding, good args, indices of the tensors read with the data
    dtype, index of a per-column parameter or None)."""
    N, H, V = 6, 64, 40
    t = lambda *s: torch.randn(*s, device=DEV).to(BF16)
    f = lambda *s: torch.randn(*s, device=DEV)
    lab = lambda: torch.randint(0, V, (N,), device=DEV)
    ext = hip_ext()
    calls = {
        "layernorm_fwd": (ext.layernorm_fwd, [t(N, H), t(H), t(H), 1e-5], [0, 1, 2], 1),
        "layernorm_fwd_residual": (ext.layernorm_fwd_residual,
                                   [t(N, H), t(N, H), t(H), t(H), 1e-5], [0, 1, 2, 3], 2),
        "rmsnorm_fwd": (ext.rmsnorm_fwd, [t(N, H), t(H), 1e-6], [0, 1], 1),
        "layernorm_bwd": (ext.layernorm_bwd, [t(N, H), t(N, H), t(H), f(N), f(N)], [1, 0, 2], 2),
        "layernorm_bwd_residual": (ext.layernorm_bwd_residual,
                                   [t(N, H), t(N, H), t(H), f(N), f(N), t(N, H)], [1, 0, 2, 5], 2),
        "rmsnorm_bwd": (ext.rmsnorm_bwd, [t(N, H), t(N, H), t(H), f(N)], [1, 0, 2], 2),
        "bias_gelu_fwd": (ext.bias_gelu_fwd, [t(N, H), t(H)], [0, 1], 1),
        "bias_gelu_bwd": (ext.bias_gelu_bwd, [t(N, H), t(N, H), t(H)], [1, 0, 2], 2),
        "colsum": (ext.colsum, [t(N, H)], [0], None),
        "grad_sumsq": (ext.grad_sumsq, [t(N, H), f(2), 0], [0], None),
        "rope_fwd": (ext.rope_fwd, [t(1, 2, N, H), f(N, H // 2), f(N, H // 2)], [0], None),
        "softmax_causal_fwd": (ext.softmax_causal_fwd, [t(1, 2, N, H), 1.0], [0], None),
        "softmax_causal_bwd": (ext.softmax_causal_bwd, [t(1, 2, N, H), t(1, 2, N, H), 1.0], [1, 0], None),
        "softmax_bias_fwd": (ext.softmax_bias_fwd, [t(2, N, H), t(1, N, H), N, 2 * N, 1.0], [0, 1], None),
        "cross_entropy_fwd": (ext.cross_entropy_fwd, [t(N, V), lab(), -100], [0], None),
        "cross_entropy_bwd": (ext.cross_entropy_bwd, [f(N), t(N, V), lab(), f(N), -100], [1], None),
        "row_max": (ext.row_max, [t(N, V)], [0], None),
        "row_sumexp": (ext.row_sumexp, [t(N, V), f(N)], [0], None),
        "gather_label_logit": (ext.gather_label_logit, [t(N, V), lab(), 0, -100], [0], None),
        "vp_ce_bwd": (ext.vp_ce_bwd, [f(N), t(N, V), lab(), f(N), 0, -100], [1], None),
        "moe_dispatch": (ext.moe_dispatch, [t(N, H), torch.randint(0, 4, (N,), device=DEV), 4, 1], [0], None),
    }
    return calls


_REFUSAL_NAMES = [
    "layernorm_fwd", "layernorm_fwd_residual", "rmsnorm_fwd", "layernorm_bwd",
    "layernorm_bwd_residual", "rmsnorm_bwd", "bias_gelu_fwd", "bias_gelu_bwd",
    "colsum", "grad_sumsq", "rope_fwd", "softmax_causal_fwd",
    "softmax_causal_bwd", "softmax_bias_fwd", "cross_entropy_fwd",
    "cross_entropy_bwd", "row_max", "row_sumexp", "gather_label_logit",
    "vp_ce_bwd", "moe_dispatch"]


def _strided(x):
    """Same values and shape, last two dims stored transposed."""
    return x.transpose(-1, -2).contiguous().transpose(-1, -2)


@pytest.mark.parametrize("name", _REFUSAL_NAMES)
def test_binding_refuses_bad_arguments(name):
    fn, good, data, wi = _refusal_calls()[name]
    fn(*good)                                   # the good call goes through
    bad_sets = []
    a = list(good)                              # an fp16 data tensor
    for i in data:
        a[i] = good[i].to(torch.float16)
    bad_sets.append(("fp16", a))
    a = list(good)                              # float64 likewise
    for i in data:
        a[i] = good[i].double()
    bad_sets.append(("fp64", a))
    a = list(good)                              # a non-contiguous input
    a[data[0]] = _strided(good[data[0]])
    assert not a[data[0]].is_contiguous()
    bad_sets.append(("strided", a))
    for i in data[1:]:                          # fp32 operand next to bf16 x
        a = list(good)
        a[i] = good[i].float()
        bad_sets.append((f"fp32 arg {i}", a))
    if wi is not None:                          # a wrong-length parameter
        a = list(good)
        a[wi] = good[wi][:-4].contiguous()
        bad_sets.append(("short w", a))
    for what, args in bad_sets:
        with pytest.raises(RuntimeError):
            fn(*args)
            pytest.fail(f"{name} accepted {what}")


def test_other_refusals():
    ext = hip_ext()
    f = lambda *s: torch.randn(*s, device=DEV)
    n = 8
    ok = [f(n), f(n), f(n), f(n).abs(), torch.Tensor(), 1e-3, 0.9, 0.95, 1e-8, 0.0, 1]
    ext.adamw_flat(*ok)
    for i, bad in [(0, f(n).to(BF16)), (1, f(n).half()), (1, f(n + 4)),
                   (2, f(n).double()), (3, f(2 * n)[::2]),
                   (4, f(n).half())]:
        a = list(ok)
        a[i] = bad
        with pytest.raises(RuntimeError):
            ext.adamw_flat(*a)
    # rope: odd D, cos of the wrong shape or dtype
    x = f(1, 2, 6, 8).to(BF16)
    cs = f(6, 4)
    ext.rope_fwd(x, cs, cs)
    for a in [(f(1, 2, 6, 7), f(6, 3), f(6, 3)), (x, f(5, 4), cs),
              (x, cs, cs.to(BF16)), (x, f(6, 8)[:, ::2], cs)]:
        with pytest.raises(RuntimeError):
            ext.rope_fwd(*a)
    # topp_select: int32 indices, fp64 u, strided probabilities
    p = torch.softmax(f(4, 32), -1).sort(-1, descending=True)
    tp, u = torch.full((4,), 0.5, device=DEV), torch.full((4,), 0.5, device=DEV)
    ext.topp_select(p.values, p.indices, tp, u)
    for a in [(p.values, p.indices.int(), tp, u), (p.values, p.indices, tp, u.double()),
              (p.values.to(BF16), p.indices, tp, u), (p.values, p.indices, tp[:3], u),
              (_strided(p.values), p.indices, tp, u)]:
        with pytest.raises(RuntimeError):
            ext.topp_select(*a)
    # labels must be int64; statistics must be fp32 and one per row
    lg, lab = f(6, 40).to(BF16), torch.randint(0, 40, (6,), device=DEV)
    with pytest.raises(RuntimeError):
        ext.cross_entropy_fwd(lg, lab.int(), -100)
    with pytest.raises(RuntimeError):
        ext.cross_entropy_bwd(f(6).to(BF16), lg, lab, f(6), -100)
    with pytest.raises(RuntimeError):
        ext.row_sumexp(lg, f(5))
    with pytest.raises(RuntimeError):
        ext.layernorm_bwd(lg, lg, f(40).to(BF16), f(6), f(7))
    with pytest.raises(RuntimeError):      # H % 4 != 0 in the backward too
        ext.layernorm_bwd(f(6, 42), f(6, 42), f(42), f(6), f(6))


# ---------------------------------------------------------------------------
# run as a script: measure the fp32 baselines on a CPU
# ---------------------------------------------------------------------------

def _measure_baselines():
    for op in (LN, LNOFF, SMC, SMB, CE, VP, BG, COLSUM, SUMSQ, ADAMW, ROPE):
        for case in op.cases:
            if op is LNOFF and case[0][0] != FP32:
                continue
            inp = op.make(case, FP32)
            eager, ref = op.ref(inp, FP32), op.ref(inp, F64)
            prefix = inp.get("_key", op.key)
            for name in ref:
                if name in ("s", "gmax", "picked"):   # compared exactly
                    continue
                if op is LNOFF and name not in ("y", "dx"):   # fixed bounds
                    continue
                _note_baseline(f"{prefix}.{name}", eager[name], ref[name])

    def up(v):          # round up to two significant digits
        if v == 0:
            return 0.0
        e = math.floor(math.log10(v)) - 1
        return float(f"{math.ceil(v / 10 ** e) * 10 ** e:.1e}")

    print(f"{'output':24s} {'rel':>9s} {'abs':>9s} {'rtol':>9s} {'atol':>9s}")
    for k, (rel, small) in sorted(_BASELINE.items()):
        print(f"{k:24s} {rel:9.2e} {small:9.2e} {up(8 * rel):9.1e} "
              f"{up(8 * small):9.1e}")
    print("FP32_TOL = {")
    for k, (rel, small) in sorted(_BASELINE.items()):
        print(f'    "{k}": ({up(8 * rel):.1e}, {up(8 * small):.1e}),')
    print("}")


if __name__ == "__main__":
    _measure_baselines()
