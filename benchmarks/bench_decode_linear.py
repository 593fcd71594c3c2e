#!/usr/bin/env python3
"""Decode-step linear microbench: ops.decode_linear (csrc/decode_linear.hip,
weights streamed once, epilogue fused) against the composition the decoder
layer runs today for the same result (F.linear through the library GEMM,
then `+ bias`, bias_gelu or the residual add as separate launches).

    python benchmarks/bench_decode_linear.py [--iters 50] [--reps 5]
    python benchmarks/bench_decode_linear.py --sweep   # kernel variants
    python benchmarks/bench_decode_linear.py --weight-dtype fp8 [--sweep]
    python benchmarks/bench_decode_linear.py --weight-dtype mxfp4 [--sweep]

Shapes: the four GPT-1.3B layer linears and the tied logits matrix
(N 50304, K 2048), each at M = 1, 4 and 16. Device-event timing around one
replay of a graph that holds `iters` calls (the decode step these linears
serve is a captured graph; --eager-launch times a stream of eager launches
instead), warm-up, the two variants alternate inside one process and the
median over the repetitions is reported. Bytes are the weight, N*K*2, so TB/s is an
ALGORITHMIC rate. Weights rotate over enough copies to exceed the 256 MiB
Infinity Cache (the footprint is printed). Needs a GPU: no CPU fallback.

--sweep times the kernel's tuning overrides (rows per workgroup, waves per
workgroup, non-temporal weight loads) against each other, alternating in the
same way; it is how the automatic choice in decode_linear.hip was made.

--weight-dtype fp8 times the fp8-weight kernel (csrc/decode_linear_fp8.hip:
e4m3 codes, one fp32 scale per output row) against the bf16 decode_linear on
the same shapes, the two alternating in one process; its bytes are N*K + 4*N.
With --sweep it sweeps the fp8 kernel's variants instead. --model 6.7B takes
the GPT-6.7B shapes (hidden 4096).

--weight-dtype mxfp4 times the MXFP4-weight kernel
(csrc/decode_linear_mxfp4.hip: e2m1 codes, one e8m0 scale per 32 elements of
K) against the fp8 kernel in the same way; its bytes are N*K/2 + N*K/32. With
--sweep it sweeps the MXFP4 kernel's variants.

--wide times the kernel for batches of 17 to 64 rows
(csrc/decode_linear_wide.hip, --weight-dtype bf16 or fp8, --ms default 32 64)
against what the op computes for such a batch without that kernel
(functional.DECODE_LINEAR_WIDE_MAX_M = 16): F.linear plus fp32 bias, GELU and
residual passes with bf16 weights, ref.decode_linear_fp8 (the fp32 twin) with
fp8 codes; the M <= 16 kernel on the first 16 rows alternates
with them to show what the x stream and the extra MFMAs cost. With --sweep it
sweeps the wide kernel's variants. --wide --weight-dtype mxfp4 times
csrc/decode_linear_wide_mxfp4.hip against the op with the wide path off (the
fp32 twin) and against the fp8 wide kernel, the three alternating; its
--sweep rows are rows per wave.

--codes times the tiled GEMM that reads codes (csrc/linear_codes.hip, M >= 65,
--weight-dtype fp8 or mxfp4, --ms default 128 256 2048) against the op with
functional.LINEAR_CODES = False (the fp32 twin, the path before that kernel)
and against F.linear on the bf16 weights plus the eager epilogue (the library
GEMM), the three alternating; it prints the achieved share of the bf16 MFMA
peak and of the HBM rate. With --sweep it sweeps the workgroup tile's N.

--ln times the LayerNorm-prologue launch (ops.decode_linear(..., ln=...)) on
the linears that follow a LayerNorm (qkv, ffn_up, logits) against the pair it
replaces, layernorm then decode_linear, alternating in the same way; with
either --weight-dtype.
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch
import torch.nn.functional as F

HBM_MEASURED_TBS = 6.29  # MI355X measured HBM read rate (TB/s)
HIDDEN = {"1.3B": 2048, "6.7B": 4096}
MS = (1, 4, 16)


def layer_shapes(H):
    """name, N, K, epilogue of the decoder layer's linears and the logits."""
    return [("qkv", 3 * H, H, "bias"), ("out_proj", H, H, "bias_res"),
            ("ffn_up", 4 * H, H, "bias_gelu"),
            ("ffn_down", H, 4 * H, "bias_res"), ("logits", 50304, H, "none")]


def num_sets(nbytes, max_sets):
    return max(2, min(max_sets, -(-(512 << 20) // nbytes)))


def time_block(fn, sets, iters, graphs=None):
    """us per call over `iters` calls rotating over the weight sets. With
    `graphs` (a dict) the calls are captured once into a graph and the graph
    is replayed: device time with the launch gaps of a captured decode step,
    free of the host's launch rate."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)

    def run():
        for i in range(iters):
            fn(sets[i % len(sets)])

    if graphs is not None and fn not in graphs:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()  # library handles and workspaces settle before capture
        torch.cuda.current_stream().wait_stream(side)
        graphs[fn] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[fn]):
            run()
    start.record()
    if graphs is not None:
        graphs[fn].replay()
    else:
        run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / iters


def alternate(fns, sets, iters, reps, captured):
    """Median us per call of each fn, the fns alternating rep by rep."""
    graphs = {} if captured else None
    for fn in fns:
        time_block(fn, sets, iters, graphs)  # warm-up
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t[i].append(time_block(fn, sets, iters, graphs))
    return [statistics.median(x) for x in t], t


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--max-sets", type=int, default=32)
    p.add_argument("--eager-launch", action="store_true",
                   help="time a stream of eager launches instead of a "
                        "captured graph: at these sizes that measures the "
                        "host's launch rate (about 9 us per launch)")
    p.add_argument("--sweep", action="store_true",
                   help="time the kernel's (rows, waves, nt) variants")
    p.add_argument("--weight-dtype", choices=("bf16", "fp8", "mxfp4"),
                   default="bf16",
                   help="fp8: the fp8-weight kernel against the bf16 one; "
                        "mxfp4: the MXFP4-weight kernel against the fp8 one")
    p.add_argument("--wide", action="store_true",
                   help="the 17 to 64 row kernel against the op's earlier "
                        "path for such batches (bf16 or fp8 weights)")
    p.add_argument("--codes", action="store_true",
                   help="the M >= 65 tiled GEMM over fp8 / mxfp4 codes "
                        "against the twin and the library GEMM")
    p.add_argument("--ln", action="store_true",
                   help="one LN + linear launch against layernorm, then "
                        "decode_linear")
    p.add_argument("--model", choices=sorted(HIDDEN), default="1.3B")
    p.add_argument("--ms", type=int, nargs="+", default=None,
                   help="batch rows (default 1 4 16; 32 64 with --wide)")
    p.add_argument("--only", nargs="+", default=None,
                   help="names of the linears to run (default all)")
    args = p.parse_args()
    if args.ms is None:
        args.ms = [128, 256, 2048] if args.codes else \
            [32, 64] if args.wide else list(MS)
    if not torch.cuda.is_available():
        sys.exit("bench_decode_linear: no GPU present (no CPU fallback)")

    from paddlefleetx_amd.ops import bias_gelu, decode_linear, hip_ext
    ext = hip_ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    bf16 = torch.bfloat16
    print(f"# decode linear microbench on {torch.cuda.get_device_name(0)}; "
          f"iters={args.iters} reps={args.reps} "
          f"{'eager launches' if args.eager_launch else 'captured'}; "
          f"bytes = N*K*2; share = of "
          f"{HBM_MEASURED_TBS} TB/s measured HBM")
    fp8 = args.weight_dtype == "fp8"
    shapes = [sh for sh in layer_shapes(HIDDEN[args.model])
              if args.only is None or sh[0] in args.only]
    if args.ln and args.weight_dtype == "mxfp4":
        sys.exit("bench_decode_linear: no LayerNorm prologue for mxfp4")
    if args.codes:
        if args.ln or args.wide or args.weight_dtype == "bf16":
            sys.exit("bench_decode_linear: --codes takes --weight-dtype fp8 "
                     "or mxfp4 and neither --ln nor --wide")
        bench_codes(ext, decode_linear, bias_gelu, shapes, dev, args)
        return
    if args.wide:
        if args.ln:
            sys.exit("bench_decode_linear: --wide takes no LayerNorm "
                     "prologue")
        if args.weight_dtype == "mxfp4":
            bench_wide_mxfp4(ext, decode_linear, shapes, dev, args)
        else:
            bench_wide(ext, decode_linear, shapes, dev, args)
        return
    if args.ln:
        bench_ln(decode_linear, shapes, dev, args)
        return
    if fp8 or args.weight_dtype == "mxfp4":
        from paddlefleetx_amd.ops import _reference as ref
        bench_fp8(ext, ref, decode_linear, shapes, dev, args, mx=not fp8)
        return
    if not args.sweep:
        print(f"{'linear':>9} {'N':>6} {'K':>5} {'M':>3} {'MiB':>7} | "
              f"{'fused us':>9} {'TB/s':>6} {'share':>6} | "
              f"{'eager us':>9} {'TB/s':>6} {'share':>6} | speedup")
    for name, N, K, ep in shapes:
        nbytes = N * K * 2
        nsets = num_sets(nbytes, args.max_sets)
        ws = [(torch.randn(N, K, device=dev) * 0.02).to(bf16)
              for _ in range(nsets)]
        bias = torch.randn(N, device=dev).to(bf16)
        for M in args.ms:
            x = torch.randn(M, K, device=dev).to(bf16)
            res = torch.randn(M, N, device=dev).to(bf16)
            b = None if ep == "none" else bias
            r = res if ep == "bias_res" else None
            act = "gelu" if ep == "bias_gelu" else None

            def fused(w):
                return decode_linear(x, w, b, r, act)

            def eager(w):
                if ep == "none":      # parallel_matmul
                    return torch.matmul(x, w.t())
                if ep == "bias":      # ColumnParallelLinear with bias
                    return F.linear(x, w, b)
                if ep == "bias_gelu":  # FFN.up + bias_gelu
                    return bias_gelu(F.linear(x, w), b)
                # RowParallelLinear: GEMM, bias after the reduce, residual
                return res + (F.linear(x, w) + b)

            with torch.no_grad():
                want = eager(ws[0]).float()
                err = (fused(ws[0]).float() - want).abs().max().item()
                # two bf16 ulps of the largest value
                assert err <= 2.0 ** -6 * want.abs().max().item(), \
                    f"variants disagree: {err}"
                if args.sweep:
                    sweep(ext, name, N, K, M, x, ws, b, r, act or "none",
                          nbytes, args)
                    continue
                (uf, ue), (t_f, t_e) = alternate(
                    (fused, eager), ws, args.iters, args.reps,
                    not args.eager_launch)
            gf, ge = nbytes / uf / 1e6, nbytes / ue / 1e6  # TB/s
            print(f"{name:>9} {N:6d} {K:5d} {M:3d} "
                  f"{nsets * nbytes / 2**20:7.1f} | "
                  f"{uf:9.2f} {gf:6.2f} {100 * gf / HBM_MEASURED_TBS:5.1f}% | "
                  f"{ue:9.2f} {ge:6.2f} {100 * ge / HBM_MEASURED_TBS:5.1f}% | "
                  f"{ue / uf:5.2f}x  (fused min/max {min(t_f):.2f}/"
                  f"{max(t_f):.2f}, eager {min(t_e):.2f}/{max(t_e):.2f}; "
                  f"worst pairing {min(t_e) / max(t_f):.2f}x; "
                  f"max|diff| {err:.4f})")
        del ws


def sweep(ext, name, N, K, M, x, ws, b, r, act, nbytes, args):
    variants = [(rows, waves, nt) for rows in (8, 16, 32)
                for waves in (4, 8) for nt in (0, 1)]

    def make(v):
        return lambda w: ext.decode_linear(x, w, b, r, act, *v)

    med, _ = alternate([make(v) for v in variants] +
                       [lambda w: ext.decode_linear(x, w, b, r, act)],
                       ws, args.iters, args.reps, not args.eager_launch)
    best = min(range(len(variants)), key=lambda i: med[i])
    cells = " ".join(f"{v[0]}/{v[1]}/{v[2]}={u:.2f}"
                     for v, u in zip(variants, med))
    print(f"{name:>9} N={N} K={K} M={M}: auto={med[-1]:.2f} us "
          f"({nbytes / med[-1] / 1e6:.2f} TB/s); best rows/waves/nt="
          f"{variants[best]} {med[best]:.2f} us | {cells}")


FP8_VARIANTS = [(rows, waves, nt) for rows in (8, 16, 32, 64)
                for waves in (4, 8) for nt in (0, 1)]


def bench_fp8(ext, ref, decode_linear, shapes, dev, args, mx=False):
    """Quantised weights against the next wider storage: fp8 against bf16,
    or (mx) MXFP4 against fp8. One weight set = (wide weight, wide scale,
    codes, scales); both kernels rotate over the same number of sets, sized
    so the SMALLER footprint still exceeds the Infinity Cache."""
    bf16 = torch.bfloat16
    new, old = ("mxfp4", "fp8") if mx else ("fp8", "bf16")
    kernel = ext.decode_linear_mxfp4 if mx else ext.decode_linear_fp8
    twin = ref.decode_linear_mxfp4 if mx else ref.decode_linear_fp8
    if not args.sweep:
        print(f"{'linear':>9} {'N':>6} {'K':>5} {'M':>3} | "
              f"{new + ' us':>8} {'TB/s':>6} {'share':>6} | "
              f"{old + ' us':>8} {'TB/s':>6} {'share':>6} | {old}/{new}")
    for name, N, K, ep in shapes:
        nb8, nb16 = N * K + 4 * N, N * K * 2
        if mx:
            nb8, nb16 = N * K // 2 + N * K // 32, nb8
        nsets = num_sets(nb8, args.max_sets)
        sets = []
        for _ in range(nsets):
            w = (torch.randn(N, K, device=dev) * 0.02).to(bf16)
            if mx:
                sets.append(ref.quantize_weight_rows(w)
                            + ref.quantize_weight_mxfp4(w))
            else:
                sets.append((w, None) + ref.quantize_weight_rows(w))
        bias = torch.randn(N, device=dev).to(bf16)
        for M in args.ms:
            x = torch.randn(M, K, device=dev).to(bf16)
            res = torch.randn(M, N, device=dev).to(bf16)
            b = None if ep == "none" else bias
            r = res if ep == "bias_res" else None
            act = "gelu" if ep == "bias_gelu" else None

            def run8(s):
                return decode_linear(x, s[2], b, r, act, weight_scale=s[3])

            def run16(s):
                return decode_linear(x, s[0], b, r, act, weight_scale=s[1])

            with torch.no_grad():
                want = twin(x, sets[0][2], sets[0][3], b, r, act).float()
                err = (run8(sets[0]).float() - want).abs().max().item()
                # two bf16 ulps of the largest value
                assert err <= 2.0 ** -6 * want.abs().max().item(), \
                    f"{new} kernel and twin disagree: {err}"
                if args.sweep:
                    a = act or "none"
                    fns = [(lambda s, v=v: kernel(
                        x, s[2], s[3], b, r, a, *v)) for v in FP8_VARIANTS]
                    fns.append(lambda s: kernel(x, s[2], s[3], b, r, a))
                    med, _ = alternate(fns, sets, args.iters, args.reps,
                                       not args.eager_launch)
                    best = min(range(len(FP8_VARIANTS)), key=lambda i: med[i])
                    cells = " ".join(f"{v[0]}/{v[1]}/{v[2]}={u:.2f}"
                                     for v, u in zip(FP8_VARIANTS, med))
                    print(f"{name:>9} N={N} K={K} M={M}: auto={med[-1]:.2f} us"
                          f" ({nb8 / med[-1] / 1e6:.2f} TB/s); best "
                          f"rows/waves/nt={FP8_VARIANTS[best]} "
                          f"{med[best]:.2f} us | {cells}", flush=True)
                    continue
                (u8, u16), (t8, t16) = alternate(
                    (run8, run16), sets, args.iters, args.reps,
                    not args.eager_launch)
            g8, g16 = nb8 / u8 / 1e6, nb16 / u16 / 1e6  # TB/s
            print(f"{name:>9} {N:6d} {K:5d} {M:3d} | "
                  f"{u8:8.2f} {g8:6.2f} {100 * g8 / HBM_MEASURED_TBS:5.1f}% | "
                  f"{u16:8.2f} {g16:6.2f} "
                  f"{100 * g16 / HBM_MEASURED_TBS:5.1f}% | "
                  f"{u16 / u8:5.2f}x  ({new} min/max {min(t8):.2f}/"
                  f"{max(t8):.2f}, {old} {min(t16):.2f}/{max(t16):.2f}; "
                  f"worst pairing {min(t16) / max(t8):.2f}x)", flush=True)
        del sets


def bench_wide(ext, decode_linear, shapes, dev, args):
    """The 17 to 64 row kernel against the parent path of the same call and
    against the M <= 16 kernel on the first 16 rows; one weight set =
    (weight, scale or None)."""
    from paddlefleetx_amd.ops import _reference as ref
    from paddlefleetx_amd.ops import functional
    wide_max = functional.DECODE_LINEAR_WIDE_MAX_M
    bf16, fp8 = torch.bfloat16, args.weight_dtype == "fp8"
    old = "twin" if fp8 else "eager"
    if not args.sweep:
        print(f"{'linear':>9} {'N':>6} {'K':>5} {'M':>3} | {'wide us':>8} "
              f"{'TB/s':>6} {'share':>6} | {old + ' us':>9} | {'M=16 us':>8} "
              f"| {old}/wide  wide/M=16")
    for name, N, K, ep in shapes:
        nbytes = N * K + 4 * N if fp8 else N * K * 2
        nsets = num_sets(nbytes, args.max_sets)
        sets = []
        for _ in range(nsets):
            w = (torch.randn(N, K, device=dev) * 0.02).to(bf16)
            sets.append(ref.quantize_weight_rows(w) if fp8 else (w, None))
        bias = torch.randn(N, device=dev).to(bf16)
        for M in args.ms:
            x = torch.randn(M, K, device=dev).to(bf16)
            res = torch.randn(M, N, device=dev).to(bf16)
            b = None if ep == "none" else bias
            r = res if ep == "bias_res" else None
            act = "gelu" if ep == "bias_gelu" else None
            x16, r16 = x[:16], (r[:16] if r is not None else None)

            def wide(s):
                return decode_linear(x, s[0], b, r, act, weight_scale=s[1])

            def narrow(s):
                return decode_linear(x16, s[0], b, r16, act,
                                     weight_scale=s[1])

            def parent(s):
                # the op with the wide kernel switched off; a captured graph
                # keeps the path its capture took
                functional.DECODE_LINEAR_WIDE_MAX_M = 16
                try:
                    return decode_linear(x, s[0], b, r, act,
                                         weight_scale=s[1])
                finally:
                    functional.DECODE_LINEAR_WIDE_MAX_M = wide_max

            with torch.no_grad():
                want = parent(sets[0]).float()
                err = (wide(sets[0]).float() - want).abs().max().item()
                # two bf16 ulps of the largest value
                assert err <= 2.0 ** -6 * want.abs().max().item(), \
                    f"wide kernel and {old} disagree: {err}"
                if args.sweep:
                    a = act or "none"
                    fns = [(lambda s, v=v: ext.decode_linear_wide(
                        x, s[0], s[1], b, r, a, *v)) for v in FP8_VARIANTS]
                    fns.append(lambda s: ext.decode_linear_wide(
                        x, s[0], s[1], b, r, a))
                    med, _ = alternate(fns, sets, args.iters, args.reps,
                                       not args.eager_launch)
                    best = min(range(len(FP8_VARIANTS)), key=lambda i: med[i])
                    cells = " ".join(f"{v[0]}/{v[1]}/{v[2]}={u:.2f}"
                                     for v, u in zip(FP8_VARIANTS, med))
                    print(f"{name:>9} N={N} K={K} M={M}: auto={med[-1]:.2f} us"
                          f" ({nbytes / med[-1] / 1e6:.2f} TB/s); best "
                          f"rows/waves/nt={FP8_VARIANTS[best]} "
                          f"{med[best]:.2f} us | {cells}", flush=True)
                    continue
                (uw, up, un), (tw, tp, _) = alternate(
                    (wide, parent, narrow), sets, args.iters, args.reps,
                    not args.eager_launch)
            gw = nbytes / uw / 1e6  # TB/s
            print(f"{name:>9} {N:6d} {K:5d} {M:3d} | {uw:8.2f} {gw:6.2f} "
                  f"{100 * gw / HBM_MEASURED_TBS:5.1f}% | {up:9.2f} | "
                  f"{un:8.2f} | {up / uw:6.2f}x {uw / un:6.2f}x  (wide "
                  f"min/max {min(tw):.2f}/{max(tw):.2f}, {old} "
                  f"{min(tp):.2f}/{max(tp):.2f}; worst pairing "
                  f"{min(tp) / max(tw):.2f}x; max|diff| {err:.4f})",
                  flush=True)
        del sets


def bench_wide_mxfp4(ext, decode_linear, shapes, dev, args):
    """The 17 to 64 row MXFP4 kernel (csrc/decode_linear_wide_mxfp4.hip)
    against the op with the wide path switched off (the fp32 twin) and
    against the fp8 wide kernel on the same matrix; one weight set = (fp8
    codes, fp8 scales, MXFP4 codes, MXFP4 scales). The sweep's rows are rows
    per WAVE: a workgroup serves waves * rows of them."""
    from paddlefleetx_amd.ops import _reference as ref
    from paddlefleetx_amd.ops import functional
    wide_max = functional.DECODE_LINEAR_WIDE_MAX_M
    bf16 = torch.bfloat16
    if not args.sweep:
        print(f"{'linear':>9} {'N':>6} {'K':>5} {'M':>3} | {'mxfp4 us':>8} "
              f"{'TB/s':>6} {'share':>6} | {'twin us':>9} | {'fp8 us':>8} "
              f"| twin/mxfp4  fp8/mxfp4")
    for name, N, K, ep in shapes:
        nbytes = N * K // 2 + N * K // 32
        nsets = num_sets(nbytes, args.max_sets)
        sets = []
        for _ in range(nsets):
            w = (torch.randn(N, K, device=dev) * 0.02).to(bf16)
            sets.append(ref.quantize_weight_rows(w)
                        + ref.quantize_weight_mxfp4(w))
        bias = torch.randn(N, device=dev).to(bf16)
        for M in args.ms:
            x = torch.randn(M, K, device=dev).to(bf16)
            res = torch.randn(M, N, device=dev).to(bf16)
            b = None if ep == "none" else bias
            r = res if ep == "bias_res" else None
            act = "gelu" if ep == "bias_gelu" else None

            def wide(s):
                return decode_linear(x, s[2], b, r, act, weight_scale=s[3])

            def fp8(s):
                return decode_linear(x, s[0], b, r, act, weight_scale=s[1])

            def parent(s):
                # the op with the wide kernels switched off; a captured graph
                # keeps the path its capture took
                functional.DECODE_LINEAR_WIDE_MAX_M = 16
                try:
                    return decode_linear(x, s[2], b, r, act,
                                         weight_scale=s[3])
                finally:
                    functional.DECODE_LINEAR_WIDE_MAX_M = wide_max

            with torch.no_grad():
                want = parent(sets[0]).float()
                err = (wide(sets[0]).float() - want).abs().max().item()
                # two bf16 ulps of the largest value
                assert err <= 2.0 ** -6 * want.abs().max().item(), \
                    f"wide mxfp4 kernel and twin disagree: {err}"
                if args.sweep:
                    a = act or "none"
                    fns = [(lambda s, v=v: ext.decode_linear_wide_mxfp4(
                        x, s[2], s[3], b, r, a, *v)) for v in FP8_VARIANTS]
                    fns.append(lambda s: ext.decode_linear_wide_mxfp4(
                        x, s[2], s[3], b, r, a))
                    med, _ = alternate(fns, sets, args.iters, args.reps,
                                       not args.eager_launch)
                    best = min(range(len(FP8_VARIANTS)), key=lambda i: med[i])
                    cells = " ".join(f"{v[0]}/{v[1]}/{v[2]}={u:.2f}"
                                     for v, u in zip(FP8_VARIANTS, med))
                    print(f"{name:>9} N={N} K={K} M={M}: auto={med[-1]:.2f} us"
                          f" ({nbytes / med[-1] / 1e6:.2f} TB/s); best "
                          f"rows/waves/nt={FP8_VARIANTS[best]} "
                          f"{med[best]:.2f} us | {cells}", flush=True)
                    continue
                (uw, up, u8), (tw, tp, t8) = alternate(
                    (wide, parent, fp8), sets, args.iters, args.reps,
                    not args.eager_launch)
            gw = nbytes / uw / 1e6  # TB/s
            print(f"{name:>9} {N:6d} {K:5d} {M:3d} | {uw:8.2f} {gw:6.2f} "
                  f"{100 * gw / HBM_MEASURED_TBS:5.1f}% | {up:9.2f} | "
                  f"{u8:8.2f} | {up / uw:6.2f}x {u8 / uw:6.2f}x  (mxfp4 "
                  f"min/max {min(tw):.2f}/{max(tw):.2f}, twin "
                  f"{min(tp):.2f}/{max(tp):.2f}, fp8 {min(t8):.2f}/"
                  f"{max(t8):.2f}; worst pairings {min(tp) / max(tw):.2f}x "
                  f"{min(t8) / max(tw):.2f}x; max|diff| {err:.4f})",
                  flush=True)
        del sets


MFMA_PEAK_TFLOPS = 2500.0  # MI355X dense bf16 matrix peak (2.5 PF/s)
CODES_TILES = (128, 64, 32)


def bench_codes(ext, decode_linear, bias_gelu, shapes, dev, args):
    """csrc/linear_codes.hip against the op with LINEAR_CODES off (the fp32
    twin) and against the library GEMM on the bf16 weights; one weight set =
    (bf16 weight, codes, scales)."""
    from paddlefleetx_amd.ops import _reference as ref
    from paddlefleetx_amd.ops import functional
    bf16, mx = torch.bfloat16, args.weight_dtype == "mxfp4"
    quant = ref.quantize_weight_mxfp4 if mx else ref.quantize_weight_rows
    if not args.sweep:
        print(f"{'linear':>9} {'N':>6} {'K':>5} {'M':>5} | {'codes us':>9} "
              f"{'%MFMA':>6} {'%HBM':>6} | {'twin us':>10} | {'lib us':>9} | "
              f"twin/codes  lib/codes")
    for name, N, K, ep in shapes:
        wbytes = N * K // 2 + N * K // 32 if mx else N * K + 4 * N
        nsets = num_sets(wbytes, min(args.max_sets, 4))
        sets = []
        for _ in range(nsets):
            w = (torch.randn(N, K, device=dev) * 0.02).to(bf16)
            sets.append((w,) + quant(w))
        bias = torch.randn(N, device=dev).to(bf16)
        for M in args.ms:
            x = torch.randn(M, K, device=dev).to(bf16)
            res = torch.randn(M, N, device=dev).to(bf16)
            b = None if ep == "none" else bias
            r = res if ep == "bias_res" else None
            act = "gelu" if ep == "bias_gelu" else None

            def codes(s):
                return decode_linear(x, s[1], b, r, act, weight_scale=s[2])

            def twin(s):
                # the op with the kernel switched off; a captured graph keeps
                # the path its capture took
                functional.LINEAR_CODES = False
                try:
                    return decode_linear(x, s[1], b, r, act,
                                         weight_scale=s[2])
                finally:
                    functional.LINEAR_CODES = True

            def lib(s):
                if ep == "none":
                    return torch.matmul(x, s[0].t())
                if ep == "bias":
                    return F.linear(x, s[0], b)
                if ep == "bias_gelu":
                    return bias_gelu(F.linear(x, s[0]), b)
                return res + (F.linear(x, s[0]) + b)

            with torch.no_grad():
                want = twin(sets[0]).float()
                err = (codes(sets[0]).float() - want).abs().max().item()
                # two bf16 ulps of the largest value
                assert err <= 2.0 ** -6 * want.abs().max().item(), \
                    f"linear_codes and twin disagree: {err}"
                if args.sweep:
                    a = act or "none"
                    fns = [(lambda s, t=t: ext.linear_codes(
                        x, s[1], s[2], b, r, a, t)) for t in CODES_TILES]
                    fns.append(lambda s: ext.linear_codes(x, s[1], s[2], b, r,
                                                          a))
                    med, _ = alternate(fns, sets, args.iters, args.reps,
                                       not args.eager_launch)
                    cells = " ".join(f"tile_n={t}: {u:.2f}"
                                     for t, u in zip(CODES_TILES, med))
                    print(f"{name:>9} N={N} K={K} M={M}: auto={med[-1]:.2f} us"
                          f" | {cells}", flush=True)
                    continue
                (uc, ut, ul), (tc, tt, tl) = alternate(
                    (codes, twin, lib), sets, args.iters, args.reps,
                    not args.eager_launch)
            flops = 2.0 * M * N * K
            nbytes = wbytes + 2 * M * K + 2 * M * N * (2 if r is not None
                                                       else 1)
            print(f"{name:>9} {N:6d} {K:5d} {M:5d} | {uc:9.2f} "
                  f"{100 * flops / uc / 1e6 / MFMA_PEAK_TFLOPS:5.1f}% "
                  f"{100 * nbytes / uc / 1e6 / HBM_MEASURED_TBS:5.1f}% | "
                  f"{ut:10.2f} | {ul:9.2f} | {ut / uc:6.2f}x {ul / uc:6.2f}x  "
                  f"(codes min/max {min(tc):.2f}/{max(tc):.2f}, twin "
                  f"{min(tt):.2f}/{max(tt):.2f}, lib {min(tl):.2f}/"
                  f"{max(tl):.2f}; worst pairings {min(tt) / max(tc):.2f}x "
                  f"{min(tl) / max(tc):.2f}x; max|diff| {err:.4f})",
                  flush=True)
        del sets


def bench_ln(decode_linear, shapes, dev, args):
    """LN folded into the linear against layernorm + decode_linear, same
    weights (bf16, or fp8 codes and scales) for both."""
    from paddlefleetx_amd.ops import _reference as ref
    from paddlefleetx_amd.ops import layernorm
    bf16, fp8 = torch.bfloat16, args.weight_dtype == "fp8"
    print(f"{'linear':>9} {'N':>6} {'K':>5} {'M':>3} | {'fused us':>9} | "
          f"{'pair us':>9} | pair/fused")
    for name, N, K, ep in shapes:
        if name not in ("qkv", "ffn_up", "logits"):
            continue
        nsets = num_sets(N * K * (1 if fp8 else 2), args.max_sets)
        sets = []
        for _ in range(nsets):
            w = (torch.randn(N, K, device=dev) * 0.02).to(bf16)
            sets.append(ref.quantize_weight_rows(w) if fp8 else (w, None))
        b = None if ep == "none" else torch.randn(N, device=dev).to(bf16)
        act = "gelu" if ep == "bias_gelu" else None
        g, beta = (torch.randn(K, device=dev).to(bf16) for _ in range(2))
        for M in args.ms:
            x = (torch.randn(M, K, device=dev) * 2 + 1).to(bf16)

            def fused(s):
                return decode_linear(x, s[0], b, None, act, weight_scale=s[1],
                                     ln=(g, beta, 1e-5))

            def pair(s):
                return decode_linear(layernorm(x, g, beta, 1e-5), s[0], b,
                                     None, act, weight_scale=s[1])

            with torch.no_grad():
                want = pair(sets[0]).float()
                err = (fused(sets[0]).float() - want).abs().max().item()
                # two bf16 ulps of the largest value
                assert err <= 2.0 ** -6 * want.abs().max().item(), \
                    f"fused and pair disagree: {err}"
                (uf, up), (t_f, t_p) = alternate(
                    (fused, pair), sets, args.iters, args.reps,
                    not args.eager_launch)
            print(f"{name:>9} {N:6d} {K:5d} {M:3d} | {uf:9.2f} | {up:9.2f} | "
                  f"{up / uf:5.2f}x  (fused min/max {min(t_f):.2f}/"
                  f"{max(t_f):.2f}, pair {min(t_p):.2f}/{max(t_p):.2f}; worst "
                  f"pairing {min(t_p) / max(t_f):.2f}x; max|diff| {err:.4f})",
                  flush=True)
        del sets


if __name__ == "__main__":
    main()
