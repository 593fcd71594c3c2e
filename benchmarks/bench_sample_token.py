#!/usr/bin/env python3
"""Sampler microbenchmark: ops.sample_token (one launch) against the sampling
tail of the eager decode loop (logits processors + softmax + topp_sampling +
where / cat / ne / and / any) on the same logits.

Device events around each call, the two variants alternating, median of
--rounds rounds of --iters calls each.

    python benchmarks/bench_sample_token.py [--vocab 50304] [--batches 1,16]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch
import torch.nn.functional as F


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--vocab", type=int, default=50304)
    p.add_argument("--batches", type=str, default="1,16")
    p.add_argument("--history", type=int, default=160)
    p.add_argument("--top-p", type=float, default=0.9)
    p.add_argument("--top-k", type=int, default=0)
    p.add_argument("--penalty", type=float, default=1.0)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available(), "the sampler benchmark needs a GPU"

    from paddlefleetx_amd.models.gpt.generation import TopKProcess
    from paddlefleetx_amd.models.gpt.processor import get_logits_processor
    from paddlefleetx_amd.ops import sample_token, topp_sampling

    dev = torch.device("cuda")
    V, L = args.vocab, args.history
    eos, pad = V - 1, 0
    print(f"# sampler bench V={V} history={L} top_p={args.top_p} "
          f"top_k={args.top_k} penalty={args.penalty}")
    for B in [int(b) for b in args.batches.split(",")]:
        torch.manual_seed(B)
        logits_bf = (3.0 * torch.randn(B, V, device=dev)).bfloat16()
        ids_buf = torch.randint(0, V - 1, (B, L + 8), device=dev)
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        u = torch.rand(B, L + 8, device=dev)
        nxt = torch.empty(B, 1, dtype=torch.long, device=dev)
        procs = get_logits_processor(min_length=L + 4, eos_token_id=eos,
                                     repetition_penalty=args.penalty)
        tp = torch.full((B,), args.top_p, device=dev)

        def fused():
            unfinished = torch.ones(B, dtype=torch.bool, device=dev)
            sample_token(logits_bf, ids_buf, lens, unfinished, u, nxt,
                         top_k=args.top_k, top_p=args.top_p,
                         repetition_penalty=args.penalty, min_length=L + 4,
                         eos_token_id=eos, pad_token_id=pad)

        def tail():
            # what GPTForGeneration.sample does per token after the forward
            unfinished = torch.ones(B, dtype=torch.bool, device=dev)
            all_ids = ids_buf[:, :L]
            logits = procs(all_ids, logits_bf.float())
            probs = F.softmax(logits, dim=-1)
            if args.top_k > 0:
                probs = TopKProcess(probs, args.top_k)
            tok, _ = topp_sampling(probs, tp)
            tok = torch.where(unfinished.unsqueeze(1), tok,
                              torch.full_like(tok, pad))
            all_ids = torch.cat([all_ids, tok], dim=-1)
            unfinished = unfinished & (tok.squeeze(1) != eos)
            return bool(unfinished.any())  # the per-token host sync

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), \
                torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1000.0 / args.iters  # us per call

        for fn in (fused, tail):  # warm up both
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        res = {"fused": [], "tail": []}
        for _ in range(args.rounds):  # alternate the variants
            res["fused"].append(timed(fused))
            res["tail"].append(timed(tail))
        mf, mt = (statistics.median(res[k]) for k in ("fused", "tail"))
        print(f"bs={B:3d}: sample_token {mf:8.1f} us   eager tail {mt:8.1f} us"
              f"   ({mt / mf:5.1f}x)   rounds fused="
              f"{[round(x, 1) for x in res['fused']]} tail="
              f"{[round(x, 1) for x in res['tail']]}")


if __name__ == "__main__":
    main()
