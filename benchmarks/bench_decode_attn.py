#!/usr/bin/env python3
"""Decode-attention kernel microbench: the fused op (csrc/decode_attention.hip)
against the composition the tuple-cache decode path runs per layer
(split/transpose + cat K + cat V + matmul + fused_softmax_causal + matmul +
transpose/reshape).

    python benchmarks/bench_decode_attn.py [--iters 50] [--reps 5]

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
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode_attn: no GPU present (no CPU fallback)")

    from paddlefleetx_amd.ops import (decode_attention, fused_softmax_causal,
                                      hip_ext)
    hip_ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    print(f"# decode attention microbench on {torch.cuda.get_device_name(0)}; "
          f"iters={args.iters} reps={args.reps}; bytes = 2*B*h*(L+1)*D*2; "
          f"share = of {HBM_MEASURED_TBS} TB/s measured HBM")
    print(f"{'B':>3} {'h':>3} {'D':>4} {'L':>5} {'MiB':>7} | "
          f"{'fused us':>9} {'GB/s':>8} {'share':>6} | "
          f"{'compose us':>10} {'GB/s':>8} {'share':>6} | speedup")
    for B, h, D, L in SWEEP:
        scale = 1.0 / math.sqrt(D)
        nbytes = kv_bytes(B, h, D, L)
        nsets = max(2, min(args.max_sets, -(-(512 << 20) // nbytes)))
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


if __name__ == "__main__":
    main()
