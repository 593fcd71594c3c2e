#!/usr/bin/env python3
"""Decode-step linear microbench: ops.decode_linear (csrc/decode_linear.hip,
weights streamed once, epilogue fused) against the composition the decoder
layer runs today for the same result (F.linear through the library GEMM,
then `+ bias`, bias_gelu or the residual add as separate launches).

    python benchmarks/bench_decode_linear.py [--iters 50] [--reps 5]
    python benchmarks/bench_decode_linear.py --sweep   # kernel variants
    python benchmarks/bench_decode_linear.py --weight-dtype fp8 [--sweep]

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
    p.add_argument("--weight-dtype", choices=("bf16", "fp8"), default="bf16",
                   help="fp8: the fp8-weight kernel against the bf16 one")
    p.add_argument("--model", choices=sorted(HIDDEN), default="1.3B")
    p.add_argument("--ms", type=int, nargs="+", default=list(MS))
    p.add_argument("--only", nargs="+", default=None,
                   help="names of the linears to run (default all)")
    args = p.parse_args()
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
    if fp8:
        from paddlefleetx_amd.ops import _reference as ref
        bench_fp8(ext, ref, decode_linear, shapes, dev, args)
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


def bench_fp8(ext, ref, decode_linear, shapes, dev, args):
    """fp8 weights against bf16 weights, one weight set = (bf16 W, codes,
    scales); both kernels rotate over the same number of sets, sized so the
    SMALLER (fp8) footprint still exceeds the Infinity Cache."""
    bf16 = torch.bfloat16
    if not args.sweep:
        print(f"{'linear':>9} {'N':>6} {'K':>5} {'M':>3} | "
              f"{'fp8 us':>8} {'TB/s':>6} {'share':>6} | "
              f"{'bf16 us':>8} {'TB/s':>6} {'share':>6} | bf16/fp8")
    for name, N, K, ep in shapes:
        nb8, nb16 = N * K + 4 * N, N * K * 2
        nsets = num_sets(nb8, args.max_sets)
        sets = []
        for _ in range(nsets):
            w = (torch.randn(N, K, device=dev) * 0.02).to(bf16)
            codes, scale = ref.quantize_weight_rows(w)
            sets.append((w, codes, scale))
        bias = torch.randn(N, device=dev).to(bf16)
        for M in args.ms:
            x = torch.randn(M, K, device=dev).to(bf16)
            res = torch.randn(M, N, device=dev).to(bf16)
            b = None if ep == "none" else bias
            r = res if ep == "bias_res" else None
            act = "gelu" if ep == "bias_gelu" else None

            def run8(s):
                return decode_linear(x, s[1], b, r, act, weight_scale=s[2])

            def run16(s):
                return decode_linear(x, s[0], b, r, act)

            with torch.no_grad():
                want = ref.decode_linear_fp8(x, sets[0][1], sets[0][2], b, r,
                                             act).float()
                err = (run8(sets[0]).float() - want).abs().max().item()
                # two bf16 ulps of the largest value
                assert err <= 2.0 ** -6 * want.abs().max().item(), \
                    f"fp8 kernel and twin disagree: {err}"
                if args.sweep:
                    a = act or "none"
                    fns = [(lambda s, v=v: ext.decode_linear_fp8(
                        x, s[1], s[2], b, r, a, *v)) for v in FP8_VARIANTS]
                    fns.append(lambda s: ext.decode_linear_fp8(
                        x, s[1], s[2], b, r, a))
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
                  f"{u16 / u8:5.2f}x  (fp8 min/max {min(t8):.2f}/"
                  f"{max(t8):.2f}, bf16 {min(t16):.2f}/{max(t16):.2f}; "
                  f"worst pairing {min(t16) / max(t8):.2f}x)", flush=True)
        del sets


if __name__ == "__main__":
    main()
