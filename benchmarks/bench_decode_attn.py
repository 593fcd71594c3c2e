#!/usr/bin/env python3
"""Decode-attention kernel microbench: the fused op (csrc/decode_attention.hip)
against the composition the tuple-cache decode path runs per layer
(split/transpose + cat K + cat V + matmul + fused_softmax_causal + matmul +
transpose/reshape).

    python benchmarks/bench_decode_attn.py [--iters 50] [--reps 5]
    python benchmarks/bench_decode_attn.py --kv-dtype fp8

With --kv-dtype fp8 the two variants are the bf16-cache kernel and the
fp8-cache kernel (csrc/decode_attention_fp8.hip, e4m3 codes + one fp32 scale
per cached row) on the same data; fp8 bytes are 2*B*h*(L+1)*(D+4).

Device-event timing, warm-up, the two variants alternate inside one process
and the median over the repetitions is reported. Bytes are the K/V the
algorithm has to read, 2*B*h*(L+1)*D*2, so GB/s is an ALGORITHMIC rate: the
composition moves several times that. Inputs rotate over enough buffer sets
to exceed the 256 MiB Infinity Cache where memory allows (the footprint is
printed; a footprint below 256 MiB is a cache-resident measurement).
Needs a GPU: there is no CPU fallback.
"""

import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

HBM_MEASURED_TBS = 6.29  # MI355X measured HBM read rate (TB/s)
SWEEP = [(B, 16, 128, L) for B in (1, 16) for L in (128, 2048)]


def kv_bytes(B, h, D, L):
    return 2 * B * h * (L + 1) * D * 2


def kv_bytes_fp8(B, h, D, L):
    return 2 * B * h * (L + 1) * (D + 4)


def num_sets(nbytes, max_sets):
    return max(2, min(max_sets, -(-(512 << 20) // nbytes)))


def time_block(fn, sets, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / iters  # us per call


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--max-sets", type=int, default=32)
    p.add_argument("--kv-dtype", choices=("bf16", "fp8"), default="bf16",
                   help="bf16: fused bf16 kernel vs the tuple-cache "
                        "composition; fp8: bf16 kernel vs fp8 kernel")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode_attn: no GPU present (no CPU fallback)")

    from paddlefleetx_amd.ops import (decode_attention, fused_softmax_causal,
                                      hip_ext)
    hip_ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if args.kv_dtype == "fp8":
        return sweep_fp8(args, dev)
    print(f"# decode attention microbench on {torch.cuda.get_device_name(0)}; "
          f"iters={args.iters} reps={args.reps}; bytes = 2*B*h*(L+1)*D*2; "
          f"share = of {HBM_MEASURED_TBS} TB/s measured HBM")
    print(f"{'B':>3} {'h':>3} {'D':>4} {'L':>5} {'MiB':>7} | "
          f"{'fused us':>9} {'GB/s':>8} {'share':>6} | "
          f"{'compose us':>10} {'GB/s':>8} {'share':>6} | speedup")
    for B, h, D, L in SWEEP:
        scale = 1.0 / math.sqrt(D)
        nbytes = kv_bytes(B, h, D, L)
        nsets = num_sets(nbytes, args.max_sets)
        sets = []
        for _ in range(nsets):
            qkv = torch.randn(B, 1, h, 3, D, device=dev).to(torch.bfloat16)
            kc = torch.randn(B, h, L + 1, D, device=dev).to(torch.bfloat16)
            vc = torch.randn(B, h, L + 1, D, device=dev).to(torch.bfloat16)
            # the tuple cache of the composed path: L cached tokens
            kt, vt = kc[:, :, :L].contiguous(), vc[:, :, :L].contiguous()
            sets.append((qkv, kc, vc, kt, vt))
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)

        def fused(s):
            return decode_attention(s[0], s[1], s[2], lens, scale=scale,
                                    max_seq_len=L + 1)

        def composed(s):
            q, k, v = s[0].view(B, 1, h, 3 * D).split(D, dim=-1)
            q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
            k = torch.cat([s[3], k], dim=2)
            v = torch.cat([s[4], v], dim=2)
            probs = fused_softmax_causal(
                torch.matmul(q, k.transpose(-1, -2)), scale)
            return torch.matmul(probs, v).transpose(1, 2).reshape(B, 1, -1)

        with torch.no_grad():
            a, b = fused(sets[0]).float(), composed(sets[0]).float()
            err = (a - b).abs().max().item()
            assert err < 3e-2, f"variants disagree: {err}"
            for fn in (fused, composed):  # warm-up
                time_block(fn, sets, args.iters)
            t_f, t_c = [], []
            for _ in range(args.reps):
                t_f.append(time_block(fused, sets, args.iters))
                t_c.append(time_block(composed, sets, args.iters))
        uf, uc = statistics.median(t_f), statistics.median(t_c)
        gf, gc = nbytes / uf / 1e3, nbytes / uc / 1e3  # GB/s
        print(f"{B:3d} {h:3d} {D:4d} {L:5d} {nsets * nbytes / 2**20:7.1f} | "
              f"{uf:9.2f} {gf:8.1f} {gf / (HBM_MEASURED_TBS * 10):5.1f}% | "
              f"{uc:10.2f} {gc:8.1f} {gc / (HBM_MEASURED_TBS * 10):5.1f}% | "
              f"{uc / uf:5.2f}x  (fused min/max {min(t_f):.2f}/{max(t_f):.2f},"
              f" compose {min(t_c):.2f}/{max(t_c):.2f}; max|diff| {err:.4f})")
        del sets


def sweep_fp8(args, dev):
    """bf16-cache kernel vs fp8-cache kernel, alternating; each variant
    rotates over its own buffer sets, sized from its own bytes."""
    from paddlefleetx_amd.ops import _reference as ref
    from paddlefleetx_amd.ops import decode_attention
    print(f"# decode attention microbench, bf16 vs fp8 KV cache, on "
          f"{torch.cuda.get_device_name(0)}; iters={args.iters} "
          f"reps={args.reps}; bytes bf16 = 2*B*h*(L+1)*D*2, fp8 = "
          f"2*B*h*(L+1)*(D+4); share = of {HBM_MEASURED_TBS} TB/s measured "
          f"HBM")
    print(f"{'B':>3} {'h':>3} {'D':>4} {'L':>5} | {'MiB':>7} "
          f"{'bf16 us':>8} {'GB/s':>8} {'share':>6} | {'MiB':>7} "
          f"{'fp8 us':>8} {'GB/s':>8} {'share':>6} | bf16/fp8")
    for B, h, D, L in SWEEP:
        scale = 1.0 / math.sqrt(D)
        nb, nf = kv_bytes(B, h, D, L), kv_bytes_fp8(B, h, D, L)
        sets_b, sets_f = [], []
        for i in range(num_sets(nf, args.max_sets)):
            qkv = torch.randn(B, 1, h, 3, D, device=dev).to(torch.bfloat16)
            kc = torch.randn(B, h, L + 1, D, device=dev).to(torch.bfloat16)
            vc = torch.randn(B, h, L + 1, D, device=dev).to(torch.bfloat16)
            k8, ks = ref.quantize_kv_rows(kc)
            v8, vs = ref.quantize_kv_rows(vc)
            sets_f.append((qkv, k8, v8, ks, vs))
            if i < num_sets(nb, args.max_sets):
                sets_b.append((qkv, kc, vc))
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)

        def bf16(s):
            return decode_attention(s[0], s[1], s[2], lens, scale=scale,
                                    max_seq_len=L + 1)

        def fp8(s):
            return decode_attention(s[0], s[1], s[2], lens, scale=scale,
                                    max_seq_len=L + 1, k_scale=s[3],
                                    v_scale=s[4])

        with torch.no_grad():
            a, b = bf16(sets_b[0]).float(), fp8(sets_f[0]).float()
            err = (a - b).abs().max().item()
            assert err < 1e-1, f"variants disagree: {err}"
            time_block(bf16, sets_b, args.iters)  # warm-up
            time_block(fp8, sets_f, args.iters)
            t_b, t_f = [], []
            for _ in range(args.reps):
                t_b.append(time_block(bf16, sets_b, args.iters))
                t_f.append(time_block(fp8, sets_f, args.iters))
        ub, uf = statistics.median(t_b), statistics.median(t_f)
        gb, gf = nb / ub / 1e3, nf / uf / 1e3  # GB/s
        print(f"{B:3d} {h:3d} {D:4d} {L:5d} | "
              f"{len(sets_b) * nb / 2**20:7.1f} {ub:8.2f} {gb:8.1f} "
              f"{gb / (HBM_MEASURED_TBS * 10):5.1f}% | "
              f"{len(sets_f) * nf / 2**20:7.1f} {uf:8.2f} {gf:8.1f} "
              f"{gf / (HBM_MEASURED_TBS * 10):5.1f}% | {ub / uf:5.2f}x  "
              f"(bf16 min/max {min(t_b):.2f}/{max(t_b):.2f}, fp8 "
              f"{min(t_f):.2f}/{max(t_f):.2f}; max|diff| {err:.4f})")
        del sets_b, sets_f


if __name__ == "__main__":
    main()
