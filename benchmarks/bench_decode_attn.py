#!/usr/bin/env python3
"""Decode-attention kernel microbench: the fused op (csrc/decode_attention.hip)
against the composition the tuple-cache decode path runs per layer
(split/transpose + cat K + cat V + matmul + fused_softmax_causal + matmul +
transpose/reshape).

    python benchmarks/bench_decode_attn.py [--iters 50] [--reps 5]
    python benchmarks/bench_decode_attn.py --kv-dtype fp8
    python benchmarks/bench_decode_attn.py --shared 16 [--splits 0,4,8]

With --kv-dtype fp8 the two variants are the bf16-cache kernel and the
fp8-cache kernel (csrc/decode_attention_fp8.hip, e4m3 codes + one fp32 scale
per cached row) on the same data; fp8 bytes are 2*B*h*(L+1)*(D+4).

With --shared G the two variants are decode_attention on the EXPANDED cache
(16 rows, each with its own copy of its prompt's K/V) and
decode_attention_shared (csrc/decode_attention_shared.hip) on P = 16/G prompts
stored once, 8 own tokens per row; effective bytes are what each variant has
to read. --splits lists forced prefix chunk counts to time (0 = the rule).

With --shared G --kv-dtype fp8 the two variants are the shared-prompt op with
a bf16 prefix and with an fp8 prefix (csrc/decode_attention_shared_fp8.hip) on
the same data, two rounds, the worst pairing reported.

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
    p.add_argument("--shared", type=int, default=0, metavar="G",
                   help="expanded-cache kernel vs the shared-prompt op, 16 "
                        "rows as 16/G prompts x G samples")
    p.add_argument("--splits", default="0",
                   help="with --shared: prefix chunk counts, comma separated")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode_attn: no GPU present (no CPU fallback)")

    from paddlefleetx_amd.ops import (decode_attention, fused_softmax_causal,
                                      hip_ext)
    hip_ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if args.shared and args.kv_dtype == "fp8":
        return sweep_shared_fp8(args, dev)
    if args.shared:
        return sweep_shared(args, dev)
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


def sweep_shared(args, dev):
    """decode_attention on the expanded cache vs decode_attention_shared,
    alternating; each variant rotates over its own buffer sets."""
    from paddlefleetx_amd.ops import decode_attention, decode_attention_shared
    G, B, h, D, own = args.shared, 16, 16, 128, 8
    assert B % G == 0, "--shared G must divide 16"
    P = B // G
    splits = [int(x) for x in args.splits.split(",")]
    print(f"# decode attention, expanded vs shared prompt (G={G}, P={P}), on "
          f"{torch.cuda.get_device_name(0)}; iters={args.iters} "
          f"reps={args.reps}; h={h} D={D}, {own} own tokens per row; bytes "
          f"expanded = 2*B*h*(L+own+1)*D*2, shared = 2*h*(P*L+B*(own+1))*D*2")
    print(f"{'G':>3} {'L':>5} {'chunks':>6} | {'MiB':>7} {'expand us':>9} "
          f"{'GB/s':>8} | {'MiB':>7} {'shared us':>9} {'GB/s':>8} | "
          f"expand/shared")
    scale = 1.0 / math.sqrt(D)
    for L in (128, 2048):
        ne = 2 * B * h * (L + own + 1) * D * 2
        ns = 2 * h * (P * L + B * (own + 1)) * D * 2
        sets_e, sets_s = [], []
        for i in range(num_sets(ne, args.max_sets)):
            qkv = torch.randn(B, 1, h, 3, D, device=dev).to(torch.bfloat16)
            kp = torch.randn(P, h, L, D, device=dev).to(torch.bfloat16)
            vp = torch.randn(P, h, L, D, device=dev).to(torch.bfloat16)
            kc = torch.randn(B, h, own + 1, D, device=dev).to(torch.bfloat16)
            vc = torch.randn(B, h, own + 1, D, device=dev).to(torch.bfloat16)
            ke = torch.cat((kp.repeat_interleave(G, 0), kc), 2).contiguous()
            ve = torch.cat((vp.repeat_interleave(G, 0), vc), 2).contiguous()
            sets_e.append((qkv, ke, ve))
            if i < num_sets(ns, args.max_sets):
                sets_s.append((qkv, kp, vp, kc, vc))
        lens = torch.full((B,), L + own, dtype=torch.int32, device=dev)
        plens = torch.full((P,), L, dtype=torch.int32, device=dev)

        def expanded(s):
            return decode_attention(s[0], s[1], s[2], lens, scale=scale,
                                    max_seq_len=L + own + 1)

        for ns_ in splits:
            def shared(s):
                return decode_attention_shared(
                    s[0], s[1], s[2], plens, s[3], s[4], lens, G, scale=scale,
                    max_prefix_len=L, num_splits=ns_)

            with torch.no_grad():
                a = expanded(sets_e[0]).float()
                b = shared(sets_s[0]).float()
                err = (a - b).abs().max().item()
                assert err < 3e-2, f"variants disagree: {err}"
                time_block(expanded, sets_e, args.iters)  # warm-up
                time_block(shared, sets_s, args.iters)
                t_e, t_s = [], []
                for _ in range(args.reps):
                    t_e.append(time_block(expanded, sets_e, args.iters))
                    t_s.append(time_block(shared, sets_s, args.iters))
            ue, us = statistics.median(t_e), statistics.median(t_s)
            print(f"{G:3d} {L:5d} {ns_:6d} | {len(sets_e) * ne / 2**20:7.1f} "
                  f"{ue:9.2f} {ne / ue / 1e3:8.1f} | "
                  f"{len(sets_s) * ns / 2**20:7.1f} {us:9.2f} "
                  f"{ns / us / 1e3:8.1f} | {ue / us:5.2f}x  (expand min/max "
                  f"{min(t_e):.2f}/{max(t_e):.2f}, shared {min(t_s):.2f}/"
                  f"{max(t_s):.2f}; max|diff| {err:.4f})")
        del sets_e, sets_s


def sweep_shared_fp8(args, dev):
    """The shared-prompt op with a bf16 prefix vs an fp8 prefix
    (csrc/decode_attention_shared_fp8.hip), alternating, two rounds; the
    ratio reported is the worst pairing (fastest bf16 median over slowest
    fp8 median). Each op's bytes are its own: the prefix 2*P*h*L*D*2 or
    2*P*h*L*(D+4), plus the rows' bf16 own tokens."""
    from paddlefleetx_amd.ops import _reference as ref
    from paddlefleetx_amd.ops import decode_attention_shared
    G, B, h, D, own = args.shared, 16, 16, 128, 8
    assert B % G == 0, "--shared G must divide 16"
    P = B // G
    splits = [int(x) for x in args.splits.split(",")]
    print(f"# shared-prompt decode attention, bf16 vs fp8 prefix (G={G}, "
          f"P={P}), on {torch.cuda.get_device_name(0)}; iters={args.iters} "
          f"reps={args.reps} rounds=2; h={h} D={D}, {own} own tokens per row")
    print(f"{'G':>3} {'L':>5} {'chunks':>6} | {'MiB':>7} {'bf16 us':>15} "
          f"{'TB/s':>5} | {'MiB':>7} {'fp8 us':>15} {'TB/s':>5} | "
          f"bf16/fp8 (worst pairing)")
    scale = 1.0 / math.sqrt(D)
    for L in (128, 2048):
        tail = 2 * h * B * (own + 1) * D * 2
        nb, nf = 2 * P * h * L * D * 2 + tail, 2 * P * h * L * (D + 4) + tail
        sets_b, sets_f = [], []
        for i in range(num_sets(nf, args.max_sets)):
            qkv = torch.randn(B, 1, h, 3, D, device=dev).to(torch.bfloat16)
            kp = torch.randn(P, h, L, D, device=dev).to(torch.bfloat16)
            vp = torch.randn(P, h, L, D, device=dev).to(torch.bfloat16)
            kc = torch.randn(B, h, own + 1, D, device=dev).to(torch.bfloat16)
            vc = torch.randn(B, h, own + 1, D, device=dev).to(torch.bfloat16)
            sets_f.append((qkv, *ref.quantize_kv_rows(kp),
                           *ref.quantize_kv_rows(vp), kc, vc))
            if i < num_sets(nb, args.max_sets):
                sets_b.append((qkv, kp, vp, kc, vc))
        lens = torch.full((B,), L + own, dtype=torch.int32, device=dev)
        plens = torch.full((P,), L, dtype=torch.int32, device=dev)
        for ns_ in splits:
            def bf16(s):
                return decode_attention_shared(
                    s[0], s[1], s[2], plens, s[3], s[4], lens, G, scale=scale,
                    max_prefix_len=L, num_splits=ns_)

            def fp8(s):
                return decode_attention_shared(
                    s[0], s[1], s[3], plens, s[5], s[6], lens, G, scale=scale,
                    max_prefix_len=L, num_splits=ns_, k_prefix_scale=s[2],
                    v_prefix_scale=s[4])

            ub, uf = [], []
            with torch.no_grad():
                err = (bf16(sets_b[0]).float()
                       - fp8(sets_f[0]).float()).abs().max().item()
                assert err < 1e-1, f"variants disagree: {err}"
                for _ in range(2):
                    time_block(bf16, sets_b, args.iters)  # warm-up
                    time_block(fp8, sets_f, args.iters)
                    t_b, t_f = [], []
                    for _ in range(args.reps):
                        t_b.append(time_block(bf16, sets_b, args.iters))
                        t_f.append(time_block(fp8, sets_f, args.iters))
                    ub.append(statistics.median(t_b))
                    uf.append(statistics.median(t_f))
            print(f"{G:3d} {L:5d} {ns_:6d} | {len(sets_b) * nb / 2**20:7.1f} "
                  f"{ub[0]:7.2f}/{ub[1]:7.2f} {nb / max(ub) / 1e6:5.2f} | "
                  f"{len(sets_f) * nf / 2**20:7.1f} {uf[0]:7.2f}/{uf[1]:7.2f} "
                  f"{nf / max(uf) / 1e6:5.2f} | {min(ub) / max(uf):5.2f}x  "
                  f"(max|diff| {err:.4f})")
        del sets_b, sets_f


if __name__ == "__main__":
    main()
